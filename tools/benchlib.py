"""What the lattice bench tools share: timing, the report, synthetic inputs, a second library, and the C calls of the fourteen lattice entries.

Importing this module opens nothing: no GPU, no library, no argument list.  Every function is handed the device and the library it works on
(open_gpu() supplies both to a tool's main()).  The positional argument list of a la_viterbi*_batch / la_alignment_posteriors* call is built
in one place, lattice_args(), from ops' entry tables and ops._face_args in the order ops._viterbi / ops._posteriors use;
tests/test_host_benchlib.py holds it to _lib.SYMBOLS and to the call ops makes, so an entry that gains an argument fails there and not on
the GPU.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time
from collections import namedtuple

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# --quick: the smallest shapes that still reach each kernel form, (B, T, L, labels per line); T >= 4 (2 L_sung + 1)
QUICK_ONE_WAVE, QUICK_MULTI_WAVE, QUICK_STRIP = (2, 160, 8, 2), (1, 400, 40, 10), (1, 4400, 520, 10)


def _package():
    """lyricalignment_amd._lib and .ops, from the tree already on sys.path (a child of ab_children: the parent's) or else from this one."""
    if ROOT not in sys.path:
        sys.path.append(ROOT)
    from lyricalignment_amd import _lib, ops
    return _lib, ops


def open_gpu(tree=ROOT):
    """The package under `tree` on GPU 0 -> (device, its library)."""
    sys.path.insert(0, tree)
    _lib, _ = _package()
    _lib.require_gpu()
    torch.cuda.set_device(0)
    return torch.device("cuda:0"), _lib.lib()


def parser(parent_lib=False, quick=False):
    """--runs, --out and, where the tool has them, --parent-lib and --quick; a tool adds what is its own."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=None)
    if parent_lib:
        ap.add_argument("--parent-lib", default="")
    if quick:
        ap.add_argument("--quick", action="store_true", help="the same legs, bit comparisons and report at the smallest shapes that reach each kernel form")
    ap.add_argument("--out", default="")
    return ap


def parse(ap, argv, runs=30):
    args = ap.parse_args(argv)
    if args.runs is None:
        args.runs = 2 if getattr(args, "quick", False) else runs
    return args


# --------------------------------------------------------------------------- timing
def time_once(fn):
    """Device events around one call, a synchronise before and after -> ms."""
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e)


def wall_once(fn):
    """Wall clock around one call with a synchronise -> ms."""
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def _fn(leg):
    """A leg is its call, or dp_leg's / posterior_leg's (call, outputs)."""
    return leg[0] if isinstance(leg, tuple) else leg


def warm_up(legs, n=3):
    """legs [(name, leg)]: every leg called n times in turn, then a synchronise."""
    for _ in range(n):
        for _, leg in legs:
            _fn(leg)()
    torch.cuda.synchronize()


def alternated(legs, runs, once=time_once, warmup=3):
    """legs [(name, leg)]: every leg warmed up, then `runs` rounds over the legs in order (call by call) -> {name: [ms, ...]}."""
    warm_up(legs, warmup)
    ts = {name: [] for name, _ in legs}
    for _ in range(runs):
        for name, leg in legs:
            ts[name].append(once(_fn(leg)))
    return ts


def stat(ts):
    return statistics.median(ts), min(ts), max(ts)


def stats_of(ts):
    """alternated()'s times -> {name: (median, min, max)}, in the legs' order."""
    return {name: stat(t) for name, t in ts.items()}


def timed(name, st, width, lead=8, digits=3):
    """The table line of one leg: name, median (min .. max)."""
    return f"{name:{width}s} {st[0]:{lead}.{digits}f} ({st[1]:.{digits}f} .. {st[2]:.{digits}f})"


# --------------------------------------------------------------------------- report
class Report:
    """say() prints a line at once and keeps it; close() writes the kept lines to --out."""

    def __init__(self, out_path=""):
        self.out_path, self.lines = out_path, []

    def say(self, line=""):
        print(line, flush=True)
        self.lines.append(line)

    def close(self):
        if self.out_path:
            os.makedirs(os.path.dirname(os.path.abspath(self.out_path)), exist_ok=True)
            with open(self.out_path, "w") as f:
                f.write("\n".join(self.lines) + "\n")


def inside(stats, parent_stats):
    """The project's noise yardstick: this build's median within the parent's own min .. max, bounds included."""
    return parent_stats[1] <= stats[0] <= parent_stats[2]


def against_parent(name, stats, parent_stats):
    """The verdict line of one leg; stats and parent_stats are stat()'s (median, min, max) of the same alternation."""
    m, (pm, plo, phi) = stats[0], parent_stats
    where = "inside" if inside(stats, parent_stats) else (f"BELOW by {plo - m:.3f} ms" if m < plo else f"ABOVE by {m - phi:.3f} ms")
    return f"{name}: {m:.3f} against the parent's {pm:.3f} ({plo:.3f} .. {phi:.3f}): {where} its min .. max ({100 * (m / pm - 1):+.1f} % of its median)"


def against_parent_processes(key, this, parent, width=16):
    """The spread form, for ab_children's result: this / parent = one list of times per process -> the three lines of `key`."""
    mt, mp = [statistics.median(t) for t in this], [statistics.median(t) for t in parent]
    spread, d = max(mp) - min(mp), statistics.median(mt) - statistics.median(mp)
    return [f"{key:>{width}}  this   " + " ".join(f"{v:8.3f}" for v in mt) + f"   median {statistics.median(mt):8.3f}",
            f"{key:>{width}}  parent " + " ".join(f"{v:8.3f}" for v in mp) + f"   median {statistics.median(mp):8.3f}   "
            f"spread between the parent's processes {spread:.3f} ({100 * spread / statistics.median(mp):.2f} %)",
            f"{'':>{width}}  difference this - parent {d:+.3f} ms ({100 * d / statistics.median(mp):+.2f} %): "
            + ("inside the parent's spread: equal" if abs(d) <= spread else
               "outside the parent's spread, FASTER" if d < 0 else "OUTSIDE the parent's spread, SLOWER: a regression")]


# --------------------------------------------------------------------------- inputs
Case = namedtuple("Case", "B T L em labels n_labels n_frames")


def case(em, labels, n_labels, n_frames):
    """One shape's inputs as the legs take them; B, T and L are the tensors' own."""
    return Case(em.shape[0], em.shape[1], labels.shape[1], em, labels, n_labels, n_frames)


def planted(B, T, L, sung, seed, device):
    """Emissions -rand * 12 - 1 with a 0.8 * 12 bonus on an even segmentation of the SUNG labels (silence between them), CPU generator."""
    g = torch.Generator().manual_seed(seed)
    em = -torch.rand((B, T, L + 1), generator=g) * 12 - 1
    seg = T // (2 * len(sung) + 1)
    for i, n in enumerate(sung):
        em[:, (2 * i + 1) * seg:(2 * i + 2) * seg, 1 + n] += 9.6
    for i in range(len(sung) + 1):
        em[:, 2 * i * seg:(2 * i + 1) * seg, 0] += 9.6
    return em.to(device)


def sheet(B, T, L, device):
    """-> labels = 1 .. L in every clip [B,L], n_labels = L [B], n_frames = T [B]; int32."""
    return (torch.arange(1, L + 1, dtype=torch.int32).repeat(B, 1).to(device), torch.full((B,), L, dtype=torch.int32, device=device),
            torch.full((B,), T, dtype=torch.int32, device=device))


def rows(row, B, device):
    """One host row (skip_from, repeat_from) for every clip -> int32 [B, len(row)]."""
    return torch.tensor([list(row)] * B, dtype=torch.int32).to(device)


def open_windows(B, T, L, device):
    """Every state's window [0, T) -> (win_lo, win_hi) int32 [B, 2L+1]."""
    return (torch.zeros((B, 2 * L + 1), dtype=torch.int32, device=device), torch.full((B, 2 * L + 1), T, dtype=torch.int32, device=device))


def starts_of(lengths):
    return [sum(lengths[:i]) for i in range(len(lengths))]


def lines_of(L, line):
    """L labels in lines of `line` (the last one shorter) -> (lengths, starts)."""
    lengths = [line] * (L // line) + ([L % line] if L % line else [])
    return lengths, starts_of(lengths)


def sung_lines(lengths, times):
    """The labels in sung order when line i is sung times[i] times in a row (0 or False: left out)."""
    return [n for a, n_chars, k in zip(starts_of(lengths), lengths, times) for n in list(range(a, a + n_chars)) * int(k)]


def anchored_windows(onsets, starts, T, L, tol_s, hop=0.02):
    """Windows of every clip from one onset anchor per line, at the frame `onsets` [B,L] has for the line's first character (a line that was
    left out, onset -1: the next line's; none after it: the last frame), each within tol_s seconds -> (win_lo, win_hi) on onsets' device."""
    _package()
    from lyricalignment_amd.utils.alignment import windows_from_anchors
    lo_rows, hi_rows = [], []
    for row in onsets.cpu().tolist():
        anchors, nxt = [], None
        for a in reversed(starts):
            nxt = row[a] if row[a] >= 0 else nxt
            anchors.append((a, (nxt if nxt is not None else T - 1) * hop, tol_s))
        lo, hi = windows_from_anchors(L, T, onset_anchors=anchors)
        lo_rows.append(lo); hi_rows.append(hi)
    return torch.tensor(lo_rows, dtype=torch.int32).to(onsets.device), torch.tensor(hi_rows, dtype=torch.int32).to(onsets.device)


# --------------------------------------------------------------------------- libraries
def load_parent(path, stems):
    """Another build of the library with the prototypes of la_<stem>[_batch], la_<stem>_workspace_bytes and la_last_error."""
    SYMBOLS = _package()[0].SYMBOLS
    L = ctypes.CDLL(os.path.abspath(path))
    names = ["la_last_error"]
    for stem in stems:
        names += [f"la_{stem}_workspace_bytes", f"la_{stem}_batch" if f"la_{stem}_batch" in SYMBOLS else f"la_{stem}"]
    for name in names:
        fn = getattr(L, name)
        fn.restype, fn.argtypes = SYMBOLS[name]
    return L


def ab_children(script, this_tree, parent_tree, rounds, runs, timeout):
    """`script --child TREE --runs N` in fresh child processes, alternated this, parent, parent, this, ...; each prints one line
    CHILD_JSON {key: [ms, ...]} -> {"this": [dict per process], "parent": [...]}.  A child that fails raises with the end of its output."""
    res = {"this": [], "parent": []}
    for r in range(rounds):
        for which in (("this", "parent") if r % 2 == 0 else ("parent", "this")):
            tree = os.path.abspath(this_tree if which == "this" else parent_tree)
            p = subprocess.run([sys.executable, os.path.abspath(script), "--child", tree, "--runs", str(runs)], capture_output=True, text=True,
                               timeout=timeout)
            line = next((l for l in p.stdout.splitlines() if l.startswith("CHILD_JSON ")), None)
            if p.returncode != 0 or line is None:
                raise RuntimeError(f"child for {tree} failed ({p.returncode}):\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
            res[which].append(json.loads(line[len("CHILD_JSON "):]))
            print(f"[ab] round {r} {which} done", flush=True)
    return res


def child_json(times):
    print("CHILD_JSON " + json.dumps(times), flush=True)


# --------------------------------------------------------------------------- calls
def workspace(lib, query, dims, device):
    """lib.<query>(*dims, &need) -> a device byte buffer of max(need, 16) bytes and `need`."""
    need = ctypes.c_size_t(0)
    rc = getattr(lib, query)(*dims, ctypes.byref(need))
    assert rc == 0, (query, rc, lib.la_last_error())
    return torch.empty((max(need.value, 16),), dtype=torch.uint8, device=device), need.value


def lattice_args(stem, c, out, frames=None, skip=None, windows=None, repeat=None, path=None, boundary_window=2, row=None, scalar=None):
    """The positional C arguments of la_<stem>_batch (frames None: a DP, which writes out's onset / offset) or la_<stem> (a sweep, asked about
    frames = the DP's (onset, offset)) up to the workspace: include/lyricalign.h's order, both penalties 0, no gamma output.  row, scalar:
    what a tile entry takes (line_start and its penalty, min_frames and max_min_frames)."""
    _lib, ops = _package()
    ptr, e, dp = _lib.ptr, ops._entry(stem), frames is None
    onset, offset = (out["onset"], out["offset"]) if dp else frames
    B, T, L, em, labels, n_labels, n_frames = c
    skip_stride = skip.stride(0) if skip is not None else (0 if dp else L + 1)             # a sweep: also span_skip_prob's pitch
    face = ops._face_args(e, skip, skip_stride, 0.0, windows, repeat, 0.0, row, scalar)
    head = (ptr(em), em.stride(0), em.stride(1), ptr(labels), labels.stride(0), ptr(n_labels), ptr(n_frames), B, T, L, ptr(onset), ptr(offset), L)
    if dp:
        return head + (ptr(out["score"]), ptr(out["status"])) + face + ((ptr(out["path"]), out["path"].stride(0)) if "path" in out else ())
    written = ("occupancy", "onset_prob", "offset_prob") + (("present", "span_skip") if e.span_out else ()) + (
        ("repeat_count", "path_prob") if e.repeats else ()) + (("visits", "in_order", "path_prob") if e.row else ()) + ("log_z", "status")
    return (head + (int(boundary_window),) + face + ((ptr(path), path.stride(0) if path is not None else 0) if e.repeats or e.row else ())
            + tuple(ptr(out.get(k)) for k in written) + (0, 0, 0))


def _leg(lib, stem, c, out, **lattice):
    """-> (fn, out): fn makes one call of the entry into `out` with a workspace of the leg's own.  The argument list is built here, once: its
    addresses stay good because fn holds every tensor behind them; only the stream is looked up per call."""
    _lib, ops = _package()
    entry = getattr(lib, f"la_{stem}_batch" if lattice.get("frames") is None else f"la_{stem}")
    dims = (c.B, c.T, c.L) + ((lattice["scalar"],) if ops._entry(stem).scalar_max is not None else ())
    ws, need = workspace(lib, f"la_{stem}_workspace_bytes", dims, c.em.device)
    args = lattice_args(stem, c, out, **lattice) + (ws.data_ptr(), need)

    def fn(_held=(c, out, lattice, ws)):
        rc = entry(*args, _lib.stream_ptr())
        assert rc == 0, (stem, rc, lib.la_last_error())
    fn.workspace_bytes = need
    return fn, out


def dp_leg(lib, stem, case, skip=None, windows=None, repeat=None, row=None, scalar=None):
    """One DP entry (stem viterbi, viterbi_spans, ..., viterbi_lines, viterbi_min_duration) of `lib` on `case` -> (fn, outputs): onset, offset,
    score, status (and path where the entry writes one), caller-owned and pre-filled with -7."""
    B, T, L, dev = case.B, case.T, case.L, case.em.device
    e = _package()[1]._entry(stem)
    full = lambda shape, dtype: torch.full(shape, -7, dtype=dtype, device=dev)
    out = dict(onset=full((B, L), torch.int32), offset=full((B, L), torch.int32), score=full((B,), torch.float64), status=full((B,), torch.int32))
    if e.repeats or e.row:
        out["path"] = full((B, T), torch.int32)
    return _leg(lib, stem, case, out, skip=skip, windows=windows, repeat=repeat, row=row, scalar=scalar)


def posterior_leg(lib, stem, case, frames, skip=None, windows=None, repeat=None, path=None, boundary_window=2, row=None, scalar=None):
    """One sweep entry (stem alignment_posteriors, alignment_posteriors_spans, ..., alignment_posteriors_lines) of `lib` on `case`, asked about
    frames = the DP's contiguous (onset, offset) (and its path) -> (fn, outputs): occupancy, onset_prob, offset_prob, log_z, status and, where
    the entry writes them, present (`visits` on the repeat lattice), span_skip, repeat_count, visits, in_order and (with a path) path_prob;
    caller-owned and pre-filled with -7."""
    B, T, L, dev = case.B, case.T, case.L, case.em.device
    e = _package()[1]._entry(stem)
    assert all(t.stride() == (L, 1) for t in frames), "onset / offset [B,L] contiguous expected"
    f32 = lambda rows_, pitch: torch.full((B, pitch), -7.0, dtype=torch.float32, device=dev)[:, :rows_]
    out = dict(occupancy=f32(L, L), onset_prob=f32(L, L), offset_prob=f32(L, L), log_z=torch.full((B,), -7.0, dtype=torch.float64, device=dev),
               status=torch.full((B,), -7, dtype=torch.int32, device=dev))
    if e.span_out:                              # span_skip_prob has the row pitch the kernel is told for skip_from
        out.update(present=f32(L, L), span_skip=f32(L + 1, max(skip.stride(0) if skip is not None else 0, L + 1)))
    if e.repeats:
        out["repeat_count"] = f32(L, L)
    if e.row:
        out.update(visits=f32(L, L), in_order=f32(L, L))
    if (e.repeats or e.row) and path is not None:   # path_prob has the row pitch of path
        out["path_prob"] = f32(T, path.stride(0))
    return _leg(lib, stem, case, out, frames=tuple(frames), skip=skip, windows=windows, repeat=repeat, path=path, boundary_window=boundary_window,
                row=row, scalar=scalar)


def same_bits(a, b, keys):
    """The outputs `keys` of two legs byte for byte."""
    return all(a[k].cpu().numpy().tobytes() == b[k].cpu().numpy().tobytes() for k in keys)


DP_OUT = ("onset", "offset", "score", "status")
POSTERIOR_OUT = ("occupancy", "onset_prob", "offset_prob", "log_z", "status")
SPAN_OUT = POSTERIOR_OUT + ("present", "span_skip")
PATH_OUT = DP_OUT + ("path",)
LINES_OUT = POSTERIOR_OUT + ("visits", "in_order", "path_prob")


PARENT = "parent commit: "


def with_parent(build, lib, parent):
    """build(lib) -> [(name, leg)]; with a parent library the same legs of it behind them, named PARENT + name."""
    return build(lib) + ([(PARENT + name, leg) for name, leg in build(parent)] if parent is not None else [])


def say_against_parent(say, legs, stats):
    """For every leg that has a PARENT twin: whether every output is the twin's byte for byte, and the verdict line of its times."""
    twins = dict(legs)
    for name, (_, out) in legs:
        if PARENT + name in twins:
            same = same_bits(out, twins[PARENT + name][1], tuple(out))
            say(f"{name}: same bits as the parent commit's: {'yes' if same else 'NO'}")
            say(against_parent(name, stats[name], stats[PARENT + name]))


def ok(out):
    """Every clip's status LA_OK."""
    return int(out["status"].abs().sum()) == 0
