"""Same-process A/B of the parent's libttl_hip.so (A, _ab/parent) and this tree's (B) on the
kernels the restatement touches: ttl_oracle_segments_packed as benchmarks/bench_oracle_validator.py
times it (segments_ms: HIP events around every 65 536-row chunk, summed; its tractogram generator,
both default sizes), the two kernels of benchmarks/bench_tracker_output.py (its kernel_times()) and
ttl_oracle_segments at the shape of config 5's training step (224 history rows of 100 points, ids,
3x3 map): device time per launch (HIP events around 200 back-to-back launches) and host time per
call of the entry point.
Both libraries are loaded into one process and alternate on the same device buffers, round by
round; one JSON line per round and side.

    python benchmarks/resampler_ab.py [rounds]
"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'benchmarks'))
from tracktolearn_amd import _lib  # noqa: E402

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 4
libs = {}
for side, path in (('A', os.path.join(ROOT, '_ab', 'parent', 'tracktolearn_amd', 'libttl_hip.so')),
                   ('B', _lib.LIB_PATH)):
    _lib._lib, _lib.LIB_PATH = None, path
    libs[side] = _lib.load()
assert libs['A']._handle != libs['B']._handle


def use(side):
    _lib._lib = libs[side]


import bench  # noqa: E402
import bench_oracle_validator as bov  # noqa: E402
import bench_tracker_output as bto  # noqa: E402
from tracktolearn_amd.experiment.oracle_validator import pack  # noqa: E402
from tracktolearn_amd.oracles.oracle import oracle_segments_packed  # noqa: E402

dev = torch.device('cuda:0')
use('B')
# tracker output: the env of bench_tracker_output.main()
n = bench.N_ACTOR
subject = bench.make_subject('c2')
env = bench.make_env(subject, 'cuda:0', 'c2')
env.seeds = bench.shard_seeds(subject[1].data, n, 0, 1)
state = env.reset(0, n)
bench.track_to_exhaustion(env, state, 7, True)
torch.cuda.synchronize()
vox = float(np.mean(np.abs(env.affine_vox2rasmm)[np.diag_indices(4)][:3]))
lo, hi = 20.0 / vox, bench.MAX_LENGTH / vox

# validator tractograms
rng = np.random.default_rng(0)
tracts = {}
for size in (65536, 1048576):
    pts, lens = bov.tractogram(size, rng)
    off = np.zeros(size + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    tracts[size] = (torch.from_numpy(pts).to(dev), torch.from_numpy(off).to(dev))
    del pts
CHUNK = 65536
dirs = torch.empty((CHUNK, 127, 3), dtype=torch.float32, device=dev)


def segments_ms(size):
    pd, od = tracts[size]
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    best = None
    for _ in range(4):                      # the first pass warms up
        ms = 0.0
        for a in range(0, size, CHUNK):
            rows = min(CHUNK, size - a)
            ev[0].record()
            oracle_segments_packed(pd, od[a:a + rows + 1], 128, dirs[:rows])
            ev[1].record()
            ev[1].synchronize()
            ms += ev[0].elapsed_time(ev[1])
        best = ms if best is None else min(best, ms)
    return round(best, 4)


hist = (torch.randn(4096, 128, 3, device=dev).cumsum(1) * 0.3 + 40).contiguous()
ids = torch.randperm(4096, device=dev)[:224].int()
seg_out = torch.empty(224, 127, 3, device=dev)
LIN = (C.c_float * 9)(0.9, 0.05, 0.0, -0.03, 1.1, 0.02, 0.01, 0.0, 0.8)


def segments_call():
    """(device us per launch, host us per call) of ttl_oracle_segments, best of 5."""
    lib = _lib.load()
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    args = (hist.data_ptr(), hist.stride(0), ids.data_ptr(), 1, 224, 100, LIN, 128,
            seg_out.data_ptr(), stream)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    dev_us = host_us = None
    for _ in range(6):                      # the first pass warms up
        torch.cuda.synchronize()
        ev[0].record()
        t0 = time.perf_counter()
        for _ in range(200):
            lib.ttl_oracle_segments(*args)
        t1 = time.perf_counter()
        ev[1].record()
        ev[1].synchronize()
        d, h = ev[0].elapsed_time(ev[1]) * 5.0, (t1 - t0) * 5e3
        dev_us = d if dev_us is None else min(dev_us, d)
        host_us = h if host_us is None else min(host_us, h)
    return round(dev_us, 3), round(host_us, 3)


for r in range(1, ROUNDS + 1):
    for side in 'AB':
        use(side)
        row = {'round': r, 'side': side,
               'segments_ms_65536': segments_ms(65536), 'segments_ms_1048576': segments_ms(1048576)}
        for name, tol in (('c02', 0.2 / vox), ('c0', 0.0)):
            k = bto.kernel_times(env, n, lo, hi, tol, 3)
            row[f'select_ms_{name}'], row[f'emit_ms_{name}'] = k['select_ms'], k['emit_ms']
        row['oracle_segments_dev_us'], row['oracle_segments_host_us'] = segments_call()
        print(json.dumps(row), flush=True)
