"""The C call of every lattice wrapper in ops.py without a GPU: lib() is a stand-in whose entries record their arguments and return 0,
and the recorded list is held, name by name, to the prototype of include/lyricalign.h -- the argument count (also against _lib.SYMBOLS),
every stride, penalty and null pointer, the workspace size the query answered, and the output pointers, which are the tensors the
wrapper returns.  CPU tensors stand for device tensors (only the is_cuda check and the stream are replaced)."""
import ctypes
import os
import re

import pytest
import torch

B, T, L = 2, 6, 3
NEED = 4096
STREAM = 0x5EED
DP = ("viterbi", "viterbi_spans", "viterbi_windows", "viterbi_lattice", "viterbi_repeats")
POST = ("alignment_posteriors", "alignment_posteriors_spans", "alignment_posteriors_windows", "alignment_posteriors_lattice",
        "alignment_posteriors_repeats", "alignment_posteriors_song")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "lyricalign.h")


def _parameters(symbol):
    """The parameter names of `int <symbol>(...)` in the header, in order, and the indices of its double parameters."""
    text = open(HEADER).read()
    decl = re.search(r"\bint\s+" + symbol + r"\s*\((.*?)\)\s*;", text, flags=re.S).group(1)
    parts = [re.sub(r"\s+", " ", p).strip() for p in decl.split(",")]
    return [re.search(r"(\w+)$", p).group(1) for p in parts], [i for i, p in enumerate(parts) if re.fullmatch(r"double \w+", p)]


class _StandIn:
    """lib(): the workspace queries record (name, shape) and answer NEED, every other entry records (name, args) and returns LA_OK."""

    def __init__(self):
        self.calls, self.queries = [], []

    def __getattr__(self, name):
        def query(*dims_and_need):
            *dims, need = dims_and_need
            self.queries.append((name, tuple(dims)))
            ctypes.cast(need, ctypes.POINTER(ctypes.c_size_t))[0] = NEED
            return 0

        def entry(*args):
            self.calls.append((name, args))
            return 0
        return query if name.endswith("_workspace_bytes") else entry


@pytest.fixture
def stand_in(monkeypatch):
    from lyricalignment_amd import ops
    fake = _StandIn()
    monkeypatch.setattr(ops, "lib", lambda: fake)
    monkeypatch.setattr(ops, "_dev", lambda t, name, dtype=None: None)
    monkeypatch.setattr(ops, "stream_ptr", lambda: STREAM)
    return fake


def _inputs():
    """Every tensor with a row pitch of its own, so that a stride in the wrong place shows."""
    i32 = dict(dtype=torch.int32)
    d = dict(em=torch.zeros((B, T + 1, L + 3))[:, :T, : L + 1], labels=torch.ones((B, L + 4), **i32)[:, :L],
             n_labels=torch.full((B,), L, **i32), n_frames=torch.full((B,), T, **i32),
             onset=torch.zeros((B, L), **i32), offset=torch.ones((B, L), **i32),
             skip_from=torch.full((B, L + 6), -1, **i32)[:, : L + 1], win_lo=torch.zeros((B, 2 * L + 8), **i32)[:, : 2 * L + 1],
             win_hi=torch.full((B, 2 * L + 8), T, **i32)[:, : 2 * L + 1], repeat_from=torch.full((B, L + 2), -1, **i32)[:, :L],
             path=torch.zeros((B, T + 5), **i32)[:, :T])
    assert len({d[k].stride(0) for k in ("em", "labels", "skip_from", "win_lo", "repeat_from", "path")}) == 6
    return d


def _takes(stem):
    return dict(spans=stem not in ("viterbi", "alignment_posteriors"), windows="windows" in stem or _general(stem), repeats=_repeats(stem))


def _general(stem):
    return stem.endswith(("_lattice", "_repeats", "_song"))


def _repeats(stem):
    return stem.endswith(("_repeats", "_song"))


def _call(stem, d, given, want_gamma=False):
    """The public wrapper of `stem` with its optional arguments given or left out -> (its result, the keyword values it was handed)."""
    from lyricalignment_amd import ops
    takes = _takes(stem)
    fn = getattr(ops, stem + "_batch" if stem in DP else stem)
    kw = {}
    if takes["spans"]:
        kw.update(skip_from=d["skip_from"] if given or stem.endswith("_spans") else None, skip_penalty=1.5)
    if takes["windows"] and (given or "windows" in stem):
        kw.update(win_lo=d["win_lo"], win_hi=d["win_hi"])
    if takes["repeats"]:
        kw.update(repeat_from=d["repeat_from"] if given else None, repeat_penalty=0.25)
        if stem in POST:
            kw.update(path=d["path"] if given else None)
    args = [d["em"], d["labels"], d["n_labels"], d["n_frames"]]
    if stem in POST:
        args += [d["onset"], d["offset"]]
        kw.update(boundary_window=3, want_gamma=want_gamma)
    return fn(*args, **kw), kw


@pytest.mark.parametrize("given", [True, False], ids=["all_given", "optional_left_out"])
@pytest.mark.parametrize("stem", DP + POST)
def test_the_c_call_of_every_lattice_wrapper(stand_in, stem, given):
    from lyricalignment_amd import _lib
    d = _inputs()
    symbol = "la_" + stem + ("_batch" if stem in DP else "")
    names, doubles = _parameters(symbol)
    for want_gamma in ((False, True) if stem in POST else (False,)):
        del stand_in.calls[:], stand_in.queries[:]
        res, kw = _call(stem, d, given, want_gamma)
        assert [name for name, _ in stand_in.calls] == [symbol]                      # one C call, of the entry's own symbol
        assert stand_in.queries == [("la_" + stem + "_workspace_bytes", (B, T, L))]
        args = stand_in.calls[0][1]
        assert len(args) == len(names) == len(_lib.SYMBOLS[symbol][1])
        assert all(type(a) is (float if i in doubles else int) for i, a in enumerate(args)), [type(a) for a in args]
        a = dict(zip(names, args))
        null = lambda t: 0 if t is None else t.data_ptr()
        pitch = lambda t, none=0: none if t is None else t.stride(0)
        want = dict(em=d["em"].data_ptr(), em_batch_stride=d["em"].stride(0), em_row_stride=d["em"].stride(1), labels=d["labels"].data_ptr(),
                    labels_stride=d["labels"].stride(0), n_labels=d["n_labels"].data_ptr(), n_frames=d["n_frames"].data_ptr(), batch=B,
                    max_frames=T, max_labels=L, out_stride=L, workspace_bytes=NEED, stream=STREAM)
        if "skip_from" in kw:                    # without rows the DP is told pitch 0, a sweep Lmax + 1: span_skip_prob's pitch
            want.update(skip_from=null(kw["skip_from"]), skip_stride=pitch(kw["skip_from"], 0 if stem in DP else L + 1), skip_penalty=1.5)
        if _takes(stem)["windows"]:
            want.update(win_lo=null(kw.get("win_lo")), win_hi=null(kw.get("win_hi")), win_stride=pitch(kw.get("win_lo")))
        if "repeat_from" in kw:
            want.update(repeat_from=null(kw["repeat_from"]), repeat_stride=pitch(kw["repeat_from"]), repeat_penalty=0.25)
        if stem == "viterbi_repeats":
            want.update(path=res[4].data_ptr(), path_stride=T)
            assert res[4].shape == (B, T) and res[4].dtype == torch.int32
        if stem in DP:
            want.update(onset=res[0].data_ptr(), offset=res[1].data_ptr(), final_score=res[2].data_ptr(), status=res[3].data_ptr())
            assert len(res) == (5 if stem == "viterbi_repeats" else 4)
            assert [(t.shape, t.dtype) for t in res[:4]] == [((B, L), torch.int32)] * 2 + [((B,), torch.float64), ((B,), torch.int32)]
        else:
            want.update(onset=d["onset"].data_ptr(), offset=d["offset"].data_ptr(), boundary_window=3, occupancy=res[0].data_ptr(),
                        onset_prob=res[1].data_ptr(), offset_prob=res[2].data_ptr(), log_z=res[3].data_ptr(), status=res[4].data_ptr())
            tail = 5
            if stem != "alignment_posteriors":
                want.update({"visits" if _repeats(stem) else "present_prob": res[5].data_ptr(), "span_skip_prob": res[6].data_ptr()})
                assert res[5].shape == (B, L) and res[6].shape == (B, L + 1)
                assert res[6].stride(0) == max(pitch(kw["skip_from"], L + 1), L + 1)     # the pitch the kernel is told for skip_from
                tail = 7
            if _repeats(stem):
                want.update(path=null(kw["path"]), path_stride=pitch(kw["path"]), repeat_count=res[7].data_ptr(), path_prob=null(res[8]))
                assert res[7].shape == (B, L) and (res[8] is None) == (kw["path"] is None)
                assert res[8] is None or (res[8].shape == (B, T) and res[8].stride(0) == kw["path"].stride(0))
                tail = 9
            gamma = res[tail] if want_gamma else None
            assert len(res) == tail + int(want_gamma) and (gamma is None or gamma.shape == (B, T, 2 * L + 1))
            want.update(gamma_out=null(gamma), gamma_batch_stride=pitch(gamma), gamma_row_stride=0 if gamma is None else gamma.stride(1))
        assert a["workspace"] != 0
        del a["workspace"]
        assert a == want, {k: (a.get(k), want.get(k)) for k in set(a) | set(want) if a.get(k) != want.get(k)}


def test_the_python_side_label_limits_and_the_checks_that_exist_once(stand_in):
    """alignment_posteriors_repeats stops at 511 labels and alignment_posteriors_song at 4095 (NotImplementedError, nothing called); the
    "go together", repeat_from and path refusals carry the name of the function that was called."""
    from lyricalignment_amd import ops
    for fn, limit, why in ((ops.alignment_posteriors_repeats, 511, "one lane per state"), (ops.alignment_posteriors_song, 4095, "8192 lattice states")):
        for n in (limit, limit + 1):
            em, lab = torch.zeros((1, 2, n + 1)), torch.ones((1, n), dtype=torch.int32)
            one, frames = torch.ones((1,), dtype=torch.int32), torch.zeros((1, n), dtype=torch.int32)
            del stand_in.calls[:]
            if n == limit:
                assert len(fn(em, lab, one, one, frames, frames)) == 9 and len(stand_in.calls) == 1
            else:
                with pytest.raises(NotImplementedError, match=f"{fn.__name__}: max_labels {n} exceeds {limit} .*{why}"):
                    fn(em, lab, one, one, frames, frames)
                assert stand_in.calls == []
    d = _inputs()
    base = (d["em"], d["labels"], d["n_labels"], d["n_frames"])
    frames = (d["onset"], d["offset"])
    for name, args in (("viterbi_lattice_batch", base), ("viterbi_repeats_batch", base), ("alignment_posteriors_lattice", base + frames),
                       ("alignment_posteriors_repeats", base + frames), ("alignment_posteriors_song", base + frames)):
        for kw in (dict(win_lo=d["win_lo"]), dict(win_hi=d["win_hi"])):
            with pytest.raises(ValueError, match=f"^{name}: win_lo and win_hi go together$"):
                getattr(ops, name)(*args, **kw)
        if "repeats" in name or "song" in name:
            with pytest.raises(ValueError, match=rf"^{name}: repeat_from \[B, >= Lmax\] with unit inner stride expected$"):
                getattr(ops, name)(*args, repeat_from=d["repeat_from"][:, : L - 1])
            with pytest.raises(ValueError, match=f"^{name}: repeat_penalty must be >= 0$"):
                getattr(ops, name)(*args, repeat_penalty=-1.0)
        if name.startswith("alignment_posteriors_") and name != "alignment_posteriors_lattice":
            with pytest.raises(ValueError, match=rf"^{name}: path \[B, >= T\] with unit inner stride expected$"):
                getattr(ops, name)(*args, path=d["path"][:, : T - 1])
    assert stand_in.calls == []
