"""Yardstick for the pronunciation scores (include/lyricalign.h la_segment_class_scores): the sequential float64 segment sums of every
candidate class, the top-k selection by a stable sort on (-score, column), the rank of the own class and the public dicts, restated in
plain numpy / Python.  The DP has its own restatements; this one starts from its onsets and offsets."""
import numpy as np


def segment_sums(em_c, onset, offset, max_frames=None):
    """em_c [T, C] float32 (one clip), one position's onset / offset -> (float64 [C] sums over t ascending in [t0, t1), t1 - t0), with
    t0 = min(onset, T) and t1 = max(t0, min(offset, T)).  An explicit sequential loop over the frames, vectorised over the candidates
    only: np.sum would add pairwise."""
    em_c = np.asarray(em_c, dtype=np.float32)
    T = em_c.shape[0] if max_frames is None else int(max_frames)
    t0 = min(int(onset), T)
    t1 = max(t0, min(int(offset), T))
    acc = np.zeros(em_c.shape[1], dtype=np.float64)
    with np.errstate(invalid="ignore"):
        for t in range(t0, t1):
            acc = acc + em_c[t].astype(np.float64)
    return acc, t1 - t0


def select(sums, own_col, top_k):
    """float64 [C] sums -> (top_col [top_k], top_score [top_k], own_score, own_rank): a stable sort on (-score, column); -1 / -inf
    beyond C entries; own_rank = the own column's place in that order (the candidates with a larger sum, or an equal sum and a smaller
    column), -1 and own_score 0 without an own column."""
    C = len(sums)
    order = sorted(range(C), key=lambda j: (-sums[j], j)) if not np.isnan(sums).any() else list(range(C))
    # (-(-inf) = +inf sorts last, as it must; equal keys keep their column order: sorted() is stable)
    top_col = [order[k] if k < C else -1 for k in range(top_k)]
    top_score = [float(sums[order[k]]) if k < C else -np.inf for k in range(top_k)]
    if own_col is None or own_col < 0 or own_col >= C:
        return top_col, top_score, 0.0, -1
    return top_col, top_score, float(sums[own_col]), order.index(own_col)


def rank_by_count(sums, own_col):
    """The rank stated as the contract does, independent of the sort: how many candidates beat the own class."""
    return sum(1 for j in range(len(sums)) if sums[j] > sums[own_col] or (sums[j] == sums[own_col] and j < own_col))


def segment_class_scores(em_c, n_labels, onset, offset, own_col, top_k, fill=None):
    """The entry restated for a batch: em_c [B, T, C], n_labels [B], onset / offset / own_col [B, Lmax] -> dict of arrays shaped as the
    entry's outputs (seg_score [B, Lmax, C], top_col / top_score [B, Lmax, top_k], own_score / own_rank / n_seg_frames [B, Lmax]).
    Entries of positions n >= n_labels[b] hold `fill[name]` (what the caller's buffers held: the entry does not write them)."""
    em_c = np.asarray(em_c, dtype=np.float32)
    B, T, C = em_c.shape
    Lmax = np.asarray(onset).shape[1]
    fill = fill or {}
    out = {"seg_score": np.full((B, Lmax, C), fill.get("seg_score", 0.0), dtype=np.float64),
           "top_col": np.full((B, Lmax, top_k), fill.get("top_col", 0), dtype=np.int32),
           "top_score": np.full((B, Lmax, top_k), fill.get("top_score", 0.0), dtype=np.float64),
           "own_score": np.full((B, Lmax), fill.get("own_score", 0.0), dtype=np.float64),
           "own_rank": np.full((B, Lmax), fill.get("own_rank", 0), dtype=np.int32),
           "n_seg_frames": np.full((B, Lmax), fill.get("n_seg_frames", 0), dtype=np.int32)}
    for b in range(B):
        for n in range(min(max(int(n_labels[b]), 0), Lmax)):
            if onset[b][n] < 0:
                out["seg_score"][b, n] = 0.0
                out["top_col"][b, n] = -1
                out["top_score"][b, n] = 0.0
                out["own_score"][b, n], out["own_rank"][b, n], out["n_seg_frames"][b, n] = 0.0, -1, 0
                continue
            sums, frames = segment_sums(em_c[b], onset[b][n], offset[b][n])
            tc, ts, own, rank = select(sums, int(own_col[b][n]), top_k)
            out["seg_score"][b, n] = sums
            out["top_col"][b, n] = tc
            out["top_score"][b, n] = ts
            out["own_score"][b, n], out["own_rank"][b, n], out["n_seg_frames"][b, n] = own, rank, frames
    return out


def candidate_classes(pronunciation_classes, label_lists):
    """The keyword's meaning: an int N = classes 1 .. N, else the ids given; the sheet's own classes unioned in; sorted and unique."""
    base = range(1, int(pronunciation_classes) + 1) if isinstance(pronunciation_classes, (int, np.integer)) else pronunciation_classes
    return sorted(set(int(c) for c in base) | set(int(c) for row in label_lists for c in row))


def pronunciation_dicts(ref, b, own_classes, classes):
    """segment_class_scores' arrays for clip b -> the public list: per position None (skipped) or {"class", "frames", "log_prob", "rank",
    "gop", "top"} with the per-frame means; own_classes[n] = the position's own class id, classes = the candidate list."""
    out = []
    for n, own in enumerate(own_classes):
        frames = int(ref["n_seg_frames"][b, n])
        if ref["own_rank"][b, n] < 0 and (ref["top_col"][b, n] < 0).all():
            out.append(None)
            continue
        own_score, best, per = float(ref["own_score"][b, n]), float(ref["top_score"][b, n, 0]), max(frames, 1)
        out.append({"class": int(own), "frames": frames, "log_prob": own_score / per, "rank": int(ref["own_rank"][b, n]),
                    "gop": 0.0 if own_score == best else (own_score - best) / per,          # (equal: also -inf beside -inf)
                    "top": [(int(classes[j]), float(s) / per) for j, s in zip(ref["top_col"][b, n], ref["top_score"][b, n]) if j >= 0]})
    return out
