"""What the same-box A/B tools share (gru_bench.py, attn_ab_bench.py, x2_ab_bench.py): a second build of the library loaded beside this one
in one process, outputs compared byte for byte, calls of the two alternated with device events around one call."""
from __future__ import annotations

import ctypes
import os
import statistics


def load_sibling(path: str, entries):
    """Another liblyricalign_hip.so with the signatures of `entries` (names in _lib.SYMBOLS) set."""
    from lyricalignment_amd._lib import SYMBOLS
    other = ctypes.CDLL(os.path.abspath(path))
    for name in entries:
        fn = getattr(other, name)
        fn.restype, fn.argtypes = SYMBOLS[name]
    return other


def same_bytes(a, b) -> bool:
    import torch
    return a.cpu().contiguous().view(torch.uint8).numpy().tobytes() == b.cpu().contiguous().view(torch.uint8).numpy().tobytes()


def time_once(fn) -> float:
    """One call between two device events, milliseconds."""
    import torch
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e)


def alternate(calls, runs: int):
    """`runs` rounds over the calls, one timed call each, the order reversed from round to round (the call after the other library's is not
    the same call) -> the times of each call."""
    ts = [[] for _ in calls]
    for r in range(runs):
        for i in (range(len(calls)) if r % 2 == 0 else reversed(range(len(calls)))):
            ts[i].append(time_once(calls[i]))
    return ts


def measure_leg(name: str, legs, runs: int, who: str):
    """legs = [(call, outputs by name) of this build, the same of the other library]: a warm-up of 3 calls each, the outputs compared, the calls
    alternated -> (bit-equal, this build's median, the other's median) in ms; prints the leg's line."""
    import torch
    for fn, _ in legs:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    equal = all(same_bytes(legs[0][1][k], legs[1][1][k]) for k in legs[0][1])
    ts = alternate([fn for fn, _ in legs], runs)
    m, pm = statistics.median(ts[0]), statistics.median(ts[1])
    print(f"{name:32s} {1e3 * m:9.1f} us ({1e3 * min(ts[0]):.1f} .. {1e3 * max(ts[0]):.1f})   against {who} {1e3 * pm:9.1f} us "
          f"({1e3 * min(ts[1]):.1f} .. {1e3 * max(ts[1]):.1f}): {100 * (m / pm - 1):+.2f} % of its median; outputs {'bit-equal' if equal else 'DIFFER'}", flush=True)
    return equal, m, pm


def verdict(got, ctl=None) -> int:
    """got / ctl = {leg: measure_leg's result} against the parent / against a copy of this build.  A leg passes when its outputs are bit-equal
    and its excess over the parent's median is no larger than the largest excess (either way round) the control shows on it.  -> exit status"""
    broken = [f"{n}: outputs differ from the parent's" for n, (eq, _, _) in got.items() if not eq]
    for n, (_, m, pm) in got.items() if ctl else ():
        margin = abs(ctl[n][1] / ctl[n][2] - 1)
        ok = m / pm - 1 <= margin
        print(f"{n:32s} excess over the parent {100 * (m / pm - 1):+.2f} %, control margin {100 * margin:.2f} %: {'passes' if ok else 'ABOVE THE MARGIN'}")
        if not ok:
            broken.append(f"{n}: {100 * (m / pm - 1):+.2f} % over the parent, control margin {100 * margin:.2f} %")
    print(f"verdict: {'every leg bit-equal' + (' and inside the control margin' if ctl else '') if not broken else 'RULE BROKEN: ' + '; '.join(broken)}")
    return 1 if broken else 0
