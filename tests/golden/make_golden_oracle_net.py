#!/usr/bin/env python3
"""Inputs and witness rows of the fused oracle network's mutation cases
(tests/ref_oracle_net.py:CASES, tests/test_oracle_net_reference.py).

No reference-tree code is involved: everything here restates this repo's own
``TransformerOracle``.  For every case the seeded model and the seeded inputs
are built, every mutant of the list is run on EVERY row -- in the fp16
emulation against the emulation, and in float64 against float64 -- and the
rows on which it shows most are kept as its witnesses.  The margin of a row is

    min(|emu_mutant - emu|, |ref64_mutant - ref64|) / tol_row

with tol_row = 4 x the spread of the CPU twins + one fp16 ulp of the score
(ref_oracle_net.row_tolerance) -- in this search with the spread of every row
raised to at least one fp16 ulp, so that a witness still holds when a further
twin (the module under autocast on the GPU) lands an ulp off on its row; a
mutant is visible when a row has margin >= 2.  The test re-evaluates each mutant on its witnesses only.  Stored:
inputs, witness indices, and the indices of the mutants no row shows
(``invisible``) -- the test states which those may be, and why.
"""
import os
import sys

import numpy as np
import scipy
import torch

torch.set_num_threads(4)

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.dont_write_bytecode = True
import ref_oracle_net as ron  # noqa: E402

N_WITNESS = 2


N_TRY = 8


def candidates(mutant, attention, tol):
    """Rows a mutant is tried on (a search heuristic, nothing more: the test
    verifies the witnesses).  A dropped key: the rows whose attention weight on
    that key -- of any query, or of query 0 in the last layer -- is largest
    relative to the row's tolerance.  Everything else: every sixteenth row (every second of a strided case)."""
    if mutant[0] == 'drop_key':
        any_query, query0 = attention[mutant[1]]
        seen = query0 if mutant[1] == len(attention) - 1 else any_query
        return torch.argsort(seen[:, mutant[2]] / tol, descending=True, stable=True)[:N_TRY]
    return torch.arange(0, len(tol), 16 if len(tol) > 64 else 2)


def margins(p, x, mutant, emu, ref64, tol):
    m = (ron.forward(p, x, emulate_fp16=True, mutant=mutant)[0] - emu).abs() / tol
    if mutant[0] != 'skip_round':       # (there is no rounding to skip in float64)
        m = torch.minimum(m, (ron.forward(p, x, mutant=mutant)[0] - ref64).abs() / tol)
    return m


def main(verbose=False):
    out = {}
    for name, cfg in ron.CASES.items():
        model = ron.case_model(cfg)
        p = ron.params(model)
        x = ron.case_rows(cfg)
        ref64 = ron.forward(p, x)[0]
        attention = []
        emu = ron.forward(p, x, emulate_fp16=True, trace=attention)[0]
        spread, tol = ron.row_tolerance(emu, ron.cpu_twins(model, p, x))
        # the search allows every row one more fp16 ulp of twin spread than the CPU twins
        # show, so that a witness survives a further twin (the module under autocast on the
        # GPU) that lands one ulp off on that row
        ulp = ron.fp16_ulp(emu)
        tol = 4 * torch.maximum(spread, ulp) + ulp
        muts = ron.case_mutants(cfg)
        wit = np.zeros((len(muts), N_WITNESS), dtype=np.int16)
        best = np.zeros(len(muts))
        for i, mutant in enumerate(muts):
            rows = candidates(mutant, attention, tol)
            m = margins(p, x[rows], mutant, emu[rows], ref64[rows], tol[rows])
            if float(m.max()) < 2.0 and mutant[0] != 'skip_round':     # unseen on the sample: every row
                rows = torch.arange(len(tol))
                m = margins(p, x, mutant, emu, ref64, tol)
            order = torch.argsort(m, descending=True, stable=True)[:N_WITNESS]
            wit[i] = rows[order].numpy()
            best[i] = float(m[order[0]])
        invisible = np.nonzero(best < 2.0)[0].astype(np.int16)
        out[name + '/x_sum'] = np.array(float(x.double().sum()))
        out[name + '/witness'] = wit
        out[name + '/invisible'] = invisible
        print(f'{name}: {len(muts)} mutants, scores {float(ref64.min()):.3f}..{float(ref64.max()):.3f}, '
              f'twin spread max {float(spread.max()):.2e}, tol_row {float(tol.min()):.2e}..'
              f'{float(tol.max()):.2e}, smallest visible margin '
              f'{best[best >= 2.0].min():.2f}, invisible: {[muts[i] for i in invisible]}')
        if verbose:
            for i in np.argsort(best)[:12]:
                print('   ', muts[i], f'{best[i]:.2f}', wit[i])
    out['versions'] = np.array([f'numpy {np.__version__}', f'scipy {scipy.__version__}',
                                f'torch {torch.__version__}'])
    path = os.path.join(os.environ.get('TTL_GOLDEN_OUT') or HERE, 'oracle_net_cases.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path) // 1024, 'KiB')


if __name__ == '__main__':
    main(verbose='-v' in sys.argv)
