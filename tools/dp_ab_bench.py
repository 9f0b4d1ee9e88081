"""A/B of the alignment DP entry points between two builds of the library in ONE process (profiles/lattice_refactor.txt).

    python tools/dp_ab_bench.py --parent-lib <liblyricalign_hip.so of a built checkout of the parent commit> [--runs 30] [--out FILE]

la_viterbi_batch and la_viterbi_spans_batch (without spans, and with four optional lines) at 32 clips x 1500 frames x 26 labels --
tools/optional_spans_bench.py's three legs on its emissions -- and both entry points on one 5389-frame, 171-label song (8 waves,
backpointer masks in the workspace).  Both libraries are loaded with ctypes; per leg their outputs are compared bit for bit, then
the two are alternated call by call (caller-owned buffers, device events around one call, a synchronise after each).  The yardstick
is the parent: a leg passes when this build's median lies inside the parent's own min .. max of the same run.
"""
import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ap = argparse.ArgumentParser()
ap.add_argument("--parent-lib", required=True)
ap.add_argument("--runs", type=int, default=30)
ap.add_argument("--out", default="")
args = ap.parse_args()
import torch
from lyricalignment_amd import _lib
from lyricalignment_amd._lib import SYMBOLS, ptr, stream_ptr
from lyricalignment_amd.utils.alignment import spans_from_lines

RUNS = args.runs
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def load(path):
    L = ctypes.CDLL(path)
    for name in ("la_viterbi_workspace_bytes", "la_viterbi_batch", "la_viterbi_spans_workspace_bytes", "la_viterbi_spans_batch", "la_last_error"):
        fn = getattr(L, name)
        fn.restype, fn.argtypes = SYMBOLS[name]
    return L


_lib.require_gpu()
torch.cuda.set_device(0)
dev = torch.device("cuda:0")
LIBS = {"parent": load(os.path.abspath(args.parent_lib)), "new": load(_lib.LIB_PATH)}


def time_once(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e)


def make_case(B, T, L, lines_, present):
    g = torch.Generator().manual_seed(B + T + L)
    em = -torch.rand((B, T, L + 1), generator=g) * 12 - 1
    skip_all = None
    if lines_:
        sung, pos = [], 0
        for n_chars, here in zip(lines_, present):
            sung += list(range(pos, pos + n_chars)) if here else []
            pos += n_chars
        seg = T // (2 * len(sung) + 1)
        for i, n in enumerate(sung):
            em[:, (2 * i + 1) * seg:(2 * i + 2) * seg, 1 + n] += 9.6
        for i in range(len(sung) + 1):
            em[:, 2 * i * seg:(2 * i + 1) * seg, 0] += 9.6
        skip_all = torch.tensor(spans_from_lines(lines_, [True] * len(lines_)), dtype=torch.int32).repeat(B, 1).to(dev)
    c = dict(B=B, T=T, L=L, em=em.to(dev), labels=torch.arange(1, L + 1, dtype=torch.int32).repeat(B, 1).to(dev),
             n_labels=torch.full((B,), L, dtype=torch.int32, device=dev), n_frames=torch.full((B,), T, dtype=torch.int32, device=dev),
             skip_none=torch.full((B, L + 1), -1, dtype=torch.int32, device=dev), skip_all=skip_all)
    return c


def runner(lib, c, skip):
    """-> (fn, outputs): one call of la_viterbi_batch (skip None) or la_viterbi_spans_batch into caller-owned buffers."""
    B, T, L, em = c["B"], c["T"], c["L"], c["em"]
    out = (torch.full((B, L), -7, dtype=torch.int32, device=dev), torch.full((B, L), -7, dtype=torch.int32, device=dev),
           torch.full((B,), -7.0, dtype=torch.float64, device=dev), torch.full((B,), -7, dtype=torch.int32, device=dev))
    need = ctypes.c_size_t(0)
    q = lib.la_viterbi_workspace_bytes if skip is None else lib.la_viterbi_spans_workspace_bytes
    assert q(B, T, L, ctypes.byref(need)) == 0
    ws = torch.empty((max(need.value, 16),), dtype=torch.uint8, device=dev)
    on, off, score, status = out

    def fn():
        if skip is None:
            rc = lib.la_viterbi_batch(ptr(em), em.stride(0), em.stride(1), ptr(c["labels"]), L, ptr(c["n_labels"]), ptr(c["n_frames"]), B, T, L,
                                      ptr(on), ptr(off), L, ptr(score), ptr(status), ptr(ws), need.value, stream_ptr())
        else:
            rc = lib.la_viterbi_spans_batch(ptr(em), em.stride(0), em.stride(1), ptr(c["labels"]), L, ptr(c["n_labels"]), ptr(c["n_frames"]), B, T, L,
                                            ptr(on), ptr(off), L, ptr(score), ptr(status), ptr(skip), L + 1, 0.0, ptr(ws), need.value, stream_ptr())
        assert rc == 0, lib.la_last_error()
    return fn, out, need.value


small = make_case(32, 1500, 26, [6, 7, 6, 7], [True, True, False, True])
song = make_case(1, 5389, 171, None, None)
LEGS = [("la_viterbi_batch 32 x 1500 x 26", small, None),
        ("la_viterbi_spans_batch, no spans, 32 x 1500 x 26", small, "skip_none"),
        ("la_viterbi_spans_batch, lines 6/7/6/7 optional, 32 x 1500 x 26", small, "skip_all"),
        ("la_viterbi_batch 1 x 5389 x 171 (8 waves, masks in the workspace)", song, None),
        ("la_viterbi_spans_batch, no spans, 1 x 5389 x 171", song, "skip_none")]

say(f"# alignment DP, parent commit's library against this one's on {torch.cuda.get_device_name(0)}: both loaded in one process, alternated call by call,")
say(f"# median (min .. max) of {RUNS} calls after a warm-up of 3, device events around one call, ms.  Outputs compared bit for bit before timing.")
all_ok = True
for name, c, skip_key in LEGS:
    skip = None if skip_key is None else c[skip_key]
    fns = {k: runner(lib, c, skip) for k, lib in LIBS.items()}
    for _ in range(3):
        for k in ("parent", "new"):
            fns[k][0]()
    torch.cuda.synchronize()
    same = all(torch.equal(a, b) for a, b in zip(fns["parent"][1], fns["new"][1])) and fns["parent"][2] == fns["new"][2]
    assert int(fns["new"][1][3].abs().sum()) == 0, "status not LA_OK"
    assert same, f"{name}: outputs differ between the two libraries"
    ts = {"parent": [], "new": []}
    for _ in range(RUNS):
        for k in ("parent", "new"):
            ts[k].append(time_once(fns[k][0]))
    mp, lp, hp = statistics.median(ts["parent"]), min(ts["parent"]), max(ts["parent"])
    mn, ln, hn = statistics.median(ts["new"]), min(ts["new"]), max(ts["new"])
    ok = lp <= mn <= hp
    all_ok &= ok
    say(f"{name}")
    say(f"    parent {mp:7.3f} ({lp:.3f} .. {hp:.3f})   new {mn:7.3f} ({ln:.3f} .. {hn:.3f})   outputs equal: {same}   "
        f"new median {'inside' if ok else ('BELOW' if mn < lp else 'ABOVE')} the parent's range")
say(f"all new medians inside the parent's own min .. max: {all_ok}")
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
