"""TrackVis (.trk) and MRtrix (.tck) tractogram files.

nibabel is absent from this image; the two formats ``ttl_track.py`` can write
(TrackToLearn/runners/ttl_track.py:178-186) are implemented from their public
specifications.  ``save`` follows what ``nib.streamlines.save(tractogram,
path, header=header)`` does with a (lazy) tractogram: points are first taken
to RAS+mm with ``tractogram.affine_to_rasmm`` and then, for .trk, to TrackVis
"voxmm" (voxel * voxel size, origin at the voxel corner) with the header's
vox->rasmm.  [recollection of nibabel's behaviour -- parity unpinned]
"""
import struct

import numpy as np

from tracktolearn_amd.tractogram import Tractogram

TRK_HEADER_SIZE = 1000


def axcodes(affine):
    """RAS axis codes of a vox->rasmm affine (closest-axis rule)."""
    R = np.asarray(affine)[:3, :3]
    codes = []
    labels = (('L', 'R'), ('P', 'A'), ('I', 'S'))
    for col in range(3):
        v = R[:, col]
        ax = int(np.argmax(np.abs(v)))
        codes.append(labels[ax][1 if v[ax] >= 0 else 0])
    return ''.join(codes)


def create_tractogram_header(affine, dimensions, voxel_sizes, voxel_order=None):
    """The dict ``dipy.io.utils.create_tractogram_header`` builds from a
    reference image (ttl_track.py:182-183)."""
    return {'voxel_to_rasmm': np.asarray(affine, dtype=np.float64),
            'dimensions': tuple(int(d) for d in dimensions[:3]),
            'voxel_sizes': tuple(float(v) for v in voxel_sizes[:3]),
            'voxel_order': voxel_order or axcodes(affine)}


def _to_rasmm(tractogram):
    A = getattr(tractogram, 'affine_to_rasmm', None)
    identity = A is None or np.array_equal(np.asarray(A), np.eye(4))
    A = None if identity else np.asarray(A, dtype=np.float64)
    for item in tractogram:
        s = np.asarray(item.streamline, dtype=np.float64)
        if A is not None:
            s = s @ A[:3, :3].T + A[:3, 3]
        yield s, item.data_for_streamline


def _trk_header(header, props, count):
    """The 1000 header bytes of a .trk with ``count`` streamlines; ``props``:
    (name, number of values) per streamline property."""
    vox2ras = np.asarray(header['voxel_to_rasmm'], dtype=np.float64)
    vs = np.asarray(header['voxel_sizes'], dtype=np.float64)
    names = []
    for k, n in props:          # nibabel names multi-valued properties k, then pads
        names += [k] + [k] * (n - 1)
    if len(names) > 10:
        raise ValueError('TRK holds at most 10 property values per streamline')
    hdr = bytearray(TRK_HEADER_SIZE)
    hdr[0:6] = b'TRACK\0'
    struct.pack_into('<3h', hdr, 6, *header['dimensions'])
    struct.pack_into('<3f', hdr, 12, *vs)
    struct.pack_into('<h', hdr, 238, len(names))
    for i, nm in enumerate(names):
        raw = nm.encode('latin1')[:19]
        hdr[240 + 20 * i:240 + 20 * i + len(raw)] = raw
    struct.pack_into('<16f', hdr, 440, *vox2ras.reshape(-1))
    order = header['voxel_order'].encode('latin1')[:3]
    hdr[948:948 + len(order)] = order
    struct.pack_into('<i', hdr, 988, count)
    struct.pack_into('<i', hdr, 992, 2)
    struct.pack_into('<i', hdr, 996, TRK_HEADER_SIZE)
    return bytes(hdr)


def save_trk(tractogram, path, header):
    vox2ras = np.asarray(header['voxel_to_rasmm'], dtype=np.float64)
    vs = np.asarray(header['voxel_sizes'], dtype=np.float64)
    ras2vox = np.linalg.inv(vox2ras)
    props = None
    count = 0
    with open(path, 'wb') as f:
        f.write(b'\0' * TRK_HEADER_SIZE)
        for s, per in _to_rasmm(tractogram):
            if props is None:
                props = [(k, int(np.asarray(v).size)) for k, v in sorted(per.items())]
            vox = s @ ras2vox[:3, :3].T + ras2vox[:3, 3]
            voxmm = ((vox + 0.5) * vs).astype('<f4')
            f.write(struct.pack('<i', len(voxmm)))
            f.write(voxmm.tobytes())
            for k, _ in props:
                f.write(np.asarray(per[k], dtype='<f4').reshape(-1).tobytes())
            count += 1
        f.seek(0)
        f.write(_trk_header(header, props or [], count))
    return count


def load_trk(path):
    """Read back a .trk: streamlines in RAS+mm, properties, header dict."""
    raw = open(path, 'rb').read()
    if raw[:5] != b'TRACK':
        raise ValueError(f'{path}: not a TRK file')
    dims = struct.unpack('<3h', raw[6:12])
    vs = np.array(struct.unpack('<3f', raw[12:24]), dtype=np.float64)
    n_scalars = struct.unpack('<h', raw[36:38])[0]
    n_props = struct.unpack('<h', raw[238:240])[0]
    names = [raw[240 + 20 * i:260 + 20 * i].split(b'\0')[0].decode('latin1')
             for i in range(n_props)]
    vox2ras = np.array(struct.unpack('<16f', raw[440:504]), dtype=np.float64).reshape(4, 4)
    n_count = struct.unpack('<i', raw[988:992])[0]
    pos = TRK_HEADER_SIZE
    lines, props = [], []
    while pos < len(raw):
        n = struct.unpack('<i', raw[pos:pos + 4])[0]
        pos += 4
        pts = np.frombuffer(raw, '<f4', n * (3 + n_scalars), pos).reshape(n, 3 + n_scalars)
        pos += 4 * n * (3 + n_scalars)
        props.append(np.frombuffer(raw, '<f4', n_props, pos).copy())
        pos += 4 * n_props
        vox = pts[:, :3].astype(np.float64) / vs - 0.5
        lines.append((vox @ vox2ras[:3, :3].T + vox2ras[:3, 3]).astype(np.float32))
    assert n_count in (0, len(lines))
    per = {}
    if n_props:
        P = np.stack(props) if props else np.zeros((0, n_props), np.float32)
        for nm in dict.fromkeys(names):
            cols = [i for i, x in enumerate(names) if x == nm]
            per[nm] = P[:, cols]
    header = {'voxel_to_rasmm': vox2ras, 'dimensions': dims, 'voxel_sizes': tuple(vs),
              'voxel_order': raw[948:951].decode('latin1'), 'nb_streamlines': n_count}
    return Tractogram(lines, per), header


def _tck_header(count):
    """The text header of a .tck with ``count`` streamlines (the count field
    is ten digits wide: the length does not depend on it)."""
    lines = ['mrtrix tracks', f'count: {count:010d}', 'datatype: Float32LE']
    # the header states its own length in the "file" entry
    body = '\n'.join(lines) + '\n'
    offset = len(body) + len('file: . ') + 12 + len('\nEND\n')
    text = body + f'file: . {offset:<12d}'.rstrip() + '\nEND\n'
    text = text.ljust(offset, '\n') if len(text) < offset else text
    return text.encode('latin1')


def save_tck(tractogram, path, header=None):
    count = 0
    chunks = []
    for s, _ in _to_rasmm(tractogram):
        chunks.append(s.astype('<f4').tobytes())
        chunks.append(np.full(3, np.nan, '<f4').tobytes())
        count += 1
    chunks.append(np.full(3, np.inf, '<f4').tobytes())
    with open(path, 'wb') as f:
        f.write(_tck_header(count))
        for c in chunks:
            f.write(c)
    return count


def load_tck(path):
    raw = open(path, 'rb').read()
    head_end = raw.index(b'END\n') + 4
    fields = dict(l.split(': ', 1) for l in raw[:head_end].decode('latin1')
                  .split('\n') if ': ' in l)
    offset = int(fields['file'].split()[1])
    data = np.frombuffer(raw, '<f4', offset=offset).reshape(-1, 3)
    lines, cur = [], 0
    for i in range(len(data)):
        if np.isinf(data[i, 0]):
            break
        if np.isnan(data[i, 0]):
            lines.append(data[cur:i].copy())
            cur = i + 1
    return Tractogram(lines, {}), fields


def save(tractogram, path, header=None):
    """``nib.streamlines.save`` for the two supported formats."""
    lower = str(path).lower()
    if lower.endswith('.trk'):
        if header is None:
            raise ValueError('a .trk file needs a reference header')
        return save_trk(tractogram, path, header)
    if lower.endswith('.tck'):
        return save_tck(tractogram, path, header)
    raise ValueError('output must be .trk or .tck')


# --------------------------------------------------------------------------
# File bodies built a batch at a time: what ``save`` writes for
# the items ``Tracker.track`` yields, restated over a packed batch.  Both
# formats are flat streams of 4-byte words whose records do not depend on
# their place in the file, so the bodies of successive batches concatenate.
# --------------------------------------------------------------------------
TRK, TCK = 0, 1                    # TTL_TRACT_FILE_* (include/ttl_hip.h)
TCK_NAN_WORD = 0x7fc00000          # the bits of np.full(3, np.nan, '<f4')


class BodyDesc(object):
    """Layout and point arithmetic of a file body: ``ttl_tract_file_desc``.
    ``pre_scale`` / ``post_scale`` are None when the step is off; ``maps`` is
    a list of at most two (3, 4) float64 affine maps, applied in order."""

    def __init__(self, fmt, n_props=0, pre_scale=None, maps=(), post_scale=None):
        self.format = int(fmt)
        self.n_props = int(n_props)
        self.pre_scale = None if pre_scale is None else float(pre_scale)
        self.maps = [np.array(m, dtype=np.float64).reshape(3, 4) for m in maps]
        self.post_scale = None if post_scale is None else \
            np.array(post_scale, dtype=np.float64).reshape(3)

    def to_c(self):
        """The ctypes struct ``ttl_tract_emit_file`` reads."""
        from tracktolearn_amd import _lib
        d = _lib.TractFileDesc()
        d.format, d.n_props, d.n_maps = self.format, self.n_props, len(self.maps)
        d.has_pre, d.has_post = self.pre_scale is not None, self.post_scale is not None
        d.pre_scale = self.pre_scale or 0.0
        for m, a in enumerate(self.maps[:2]):
            d.maps[m][:] = a.reshape(-1).tolist()
        if self.post_scale is not None:
            d.post_scale[:] = self.post_scale.tolist()
        return d


def _is_identity(A):
    return A is None or np.array_equal(np.asarray(A), np.eye(4))


def body_desc(ext, affine_vox2rasmm, vox_size, header=None, n_props=0):
    """The descriptor of the file ``save(tracker.track(env, fmt), path,
    header)`` writes, points starting in the env's voxel space:
    .trk: ``to_file_space`` ((p + 0.5) * vox_size, float32 in place), the
    tractogram's ``affine_to_rasmm`` (= ``affine_vox2rasmm``; skipped, as the
    writer skips it, when it is the identity), the header's rasmm -> voxel and
    the corner-origin voxmm scaling;
    .tck: the reference's row-vector product (the transposed 3 x 3 block with
    the untransposed translation), then ``affine_to_rasmm``."""
    A = np.asarray(affine_vox2rasmm, dtype=np.float64)
    to_rasmm = [] if _is_identity(A) else [A[:3, :4]]
    if ext == '.trk':
        if header is None:
            raise ValueError('a .trk file needs a reference header')
        ras2vox = np.linalg.inv(np.asarray(header['voxel_to_rasmm'], dtype=np.float64))
        return BodyDesc(TRK, n_props, pre_scale=vox_size, maps=to_rasmm + [ras2vox[:3, :4]],
                        post_scale=header['voxel_sizes'])
    if ext == '.tck':
        first = np.concatenate((A[:3, :3].T, A[:3, 3:4]), axis=1)
        return BodyDesc(TCK, n_props, maps=[first] + to_rasmm)
    raise ValueError('output must be .trk or .tck')


def body_words(desc, k, M):
    """Words of the body of k streamlines with M points: ``ttl_tract_file_words``."""
    if desc.format == TRK:
        return k * (1 + desc.n_props) + 3 * M
    return 3 * (M + k)


def packed_body(points, counts, seeds, desc):
    """The file body of a packed batch as uint32 words: ``points`` (M, 3)
    float32, ``counts`` (k,) points per streamline, ``seeds`` (k, 3) float64
    or None.  The specification ``ttl_tract_emit_file`` equals bit for bit,
    and the path of host tensors.  Element-wise expressions only, in the order
    include/ttl_hip.h states -- no matrix product, whose summation order and
    fusing are the BLAS's choice."""
    if desc.format not in (TRK, TCK):
        raise ValueError('unknown format')
    if desc.n_props not in (0, 3) or (desc.n_props == 3 and seeds is None):
        raise ValueError('n_props is 0, or 3 with seeds')
    if len(desc.maps) > 2:
        raise ValueError('at most two affine maps')
    p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
    counts = np.asarray(counts, dtype=np.int64).reshape(-1)
    k, M = len(counts), len(p)
    if int(counts.sum()) != M:
        raise ValueError('counts do not add up to the number of points')
    if desc.pre_scale is not None:
        q = ((p + np.float32(0.5)).astype(np.float64) * desc.pre_scale).astype(np.float32)
        v = q.astype(np.float64)
    else:
        v = p.astype(np.float64)
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    for m in desc.maps:
        x, y, z = [((x * m[i, 0] + y * m[i, 1]) + z * m[i, 2]) + m[i, 3] for i in range(3)]
    if desc.post_scale is not None:
        x, y, z = [(c + 0.5) * desc.post_scale[i] for i, c in enumerate((x, y, z))]
    f = np.stack((x, y, z), axis=1).astype('<f4').view(np.uint32)
    trk = desc.format == TRK
    P = desc.n_props if trk else 0
    words = np.empty(body_words(desc, k, M), dtype=np.uint32)
    ends = np.cumsum(counts)
    b = ends - counts
    rows = np.arange(k, dtype=np.int64)
    start = rows * (1 + P) + 3 * b if trk else 3 * (b + rows)
    if trk:
        words[start] = counts.astype(np.int32).view(np.uint32)
        start = start + 1
    # point j of the batch lies 3 j words after its streamline's shift
    shift = np.repeat(start - 3 * b, counts)
    at = shift[:, None] + 3 * np.arange(M, dtype=np.int64)[:, None] + np.arange(3)
    words[at] = f
    tail = (start + 3 * counts)[:, None] + np.arange(3)
    if not trk:
        words[tail] = TCK_NAN_WORD
    elif P == 3:
        s = np.asarray(seeds, dtype=np.float64).reshape(k, 3)
        words[tail] = (s - 0.5).astype('<f4').view(np.uint32)
    return words


class PackedWriter(object):
    """Streams batch bodies (``packed_body`` / ``ttl_tract_emit_file``) into a
    .trk / .tck with the header bytes ``save_trk`` / ``save_tck`` write: one
    ``write`` per batch, the count patched in at ``close``."""

    def __init__(self, path, ext, header=None, n_props=0):
        if ext not in ('.trk', '.tck'):
            raise ValueError('output must be .trk or .tck')
        if ext == '.trk' and header is None:
            raise ValueError('a .trk file needs a reference header')
        self.ext, self.header, self.count = ext, header, 0
        self.n_props = int(n_props) if ext == '.trk' else 0
        self.words_per_row = 1 + self.n_props if ext == '.trk' else 3
        self._f = open(path, 'wb')
        self._f.write(self._head())

    def _head(self):
        if self.ext == '.tck':
            return _tck_header(self.count)
        # save_trk takes the property names from its first item: none without one
        props = [('seeds', self.n_props)] if self.n_props and self.count else []
        return _trk_header(self.header, props, self.count)

    def append(self, words, k):
        """Add the body of a batch of k streamlines (uint32 / int32 words)."""
        words = np.ascontiguousarray(words).reshape(-1)
        if words.dtype.itemsize != 4:
            raise ValueError('a file body is made of 4-byte words')
        if (len(words) - int(k) * self.words_per_row) % 3 or len(words) < k * self.words_per_row:
            raise ValueError('not the body of {} streamlines'.format(k))
        self._f.write(words.astype(words.dtype.newbyteorder('<'), copy=False).data)
        self.count += int(k)

    def close(self):
        """Finish the file; returns the number of streamlines."""
        if self._f is not None:
            if self.ext == '.tck':
                self._f.write(np.full(3, np.inf, '<f4').tobytes())
            self._f.seek(0)
            self._f.write(self._head())
            self._f.close()
            self._f = None
        return self.count

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
