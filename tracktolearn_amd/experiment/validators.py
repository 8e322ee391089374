"""Validator base class (TrackToLearn/experiment/validators.py): a named
callable that scores a validation tractogram and returns a dict of scalars."""


class Validator(object):

    def __init__(self):
        self.name = ''

    def __call__(self, filename, env):
        raise NotImplementedError('a Validator subclass scores the tractogram')
