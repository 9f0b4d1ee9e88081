"""The build's counterpart of the reference's evaluation glue (inference_alignment.align_and_evaluate,
inference_alignment.py:126-180, and inference_alignment_nogt.py:130-178): per-batch label mapping, forward,
Viterbi, MAE averaging.  Reproduces, on purpose:
  (1) class = pinyin_lookup_table[token_pinyin[token_id]] for every token id != -100 (:149-152)
  (2) batches whose ground truth is (None,) are skipped (:156-157)
  (3) avg_mae = sum(per-batch get_mae) / #evaluated batches  -- a mean of per-batch means (:172-177)
so the sharded evaluation keeps batch composition and averages the gathered per-batch values.
The alignment itself goes through AlignModel.align (fused HIP path) or, with two_step=True, through the
drop-in frame_manual_forward + perform_viterbi(_ctc) pair exactly like the reference's loop.
"""
from __future__ import annotations

import math
import re
from typing import Any, Iterable, List, Optional, Sequence

import numpy as np
import torch

from .sharding import map_sharded
from .utils.alignment import get_mae, perform_viterbi, perform_viterbi_ctc


class PinyinClassLUT:
    """Vectorised form of the reference's Python double loop: a [n_tokens] int table token id -> class id."""

    def __init__(self, token_pinyin: Sequence[str], pinyin_lookup_table: dict):
        self.table = np.asarray([pinyin_lookup_table[p] for p in token_pinyin], dtype=np.int64)
        self.lookup = dict(pinyin_lookup_table)
        self.syllables = {}                      # class id -> syllable: the first syllable of the lookup table that maps to the class
        for syllable, c in self.lookup.items():
            self.syllables.setdefault(int(c), syllable)

    def syllable_of(self, class_id: int) -> str:
        """The syllable of a class id (the inverse of pinyin_lookup_table; KeyError for an id the table does not hold)."""
        return self.syllables[int(class_id)]

    def __call__(self, tokens) -> torch.Tensor:
        t = torch.as_tensor(tokens).clone().long()
        keep = t != -100
        t[keep] = torch.from_numpy(self.table)[t[keep]]
        return t

    def readings_of(self, tokens, heteronyms) -> List[list]:
        """Characters with several readings (addition; the table holds one syllable per character): tokens [B, L] token ids with -100 padding,
        heteronyms = {token id: [syllable, ...]}, a caller-supplied dict of the further syllables a character may be sung as, resolved
        through pinyin_lookup_table -> AlignModel.align's `alternatives`: per row the list of (position among the row's labels, [class id,
        ...]) for every character with at least one class beside its own (the table's class and repeats are dropped).  ValueError for a
        syllable the lookup table does not hold."""
        out = []
        for row in torch.as_tensor(tokens).long().tolist():
            alts, n = [], 0
            for tok in row:
                if tok == -100:
                    continue
                own, extras = int(self.table[tok]), []
                for syllable in heteronyms.get(tok, ()):
                    if syllable not in self.lookup:
                        raise ValueError(f"readings_of: syllable {syllable!r} of token {tok} is not in the pinyin lookup table")
                    c = int(self.lookup[syllable])
                    if c != own and c not in extras:
                        extras.append(c)
                if extras:
                    alts.append((n, extras))
                n += 1
            out.append(alts)
        return out


PER_CLIP_MAX_SAMPLES = 3000 * 160 + 159        # the longest clip AlignModel.align(per_clip=True) takes: 3000 mel frames = 30 s


def _evaluate_grouped(model, batches: Sequence[Any], lut, use_ctc_loss: bool, group: int):
    """evaluate_batches' per-batch MAEs with `group` consecutive evaluated one-clip batches per device call (per_clip=True: every clip
    as if it ran alone).  Clips longer than 30 s go alone through the dense call, as with group = 1."""
    maes: List[Optional[float]] = [None] * len(batches)
    todo = []
    for i, (audios, tokens, _, onset_offset, _, _) in enumerate(batches):
        if len(audios) != 1:
            raise ValueError(f"evaluate_batches(group={group}): batch {i} holds {len(audios)} clips; grouping is defined for one-clip batches "
                             "(the reference couples the clips of a larger batch)")
        labels = lut(tokens) if lut is not None else torch.as_tensor(tokens)
        if onset_offset == (None,):
            continue
        todo.append((i, audios[0], labels, onset_offset))

    def flush(items):
        if not items:
            return
        rows = [[int(v) for v in torch.as_tensor(lab)[0].tolist() if int(v) != -100] for _, _, lab, _ in items]
        res = model.align([a for _, a, _, _ in items], rows, use_ctc=use_ctc_loss, per_clip=True)
        for (i, _, _, gt), r in zip(items, res):
            maes[i] = get_mae(gt, [r])

    pending = []
    for item in todo:
        if len(item[1]) > PER_CLIP_MAX_SAMPLES:
            maes[item[0]] = get_mae(item[3], model.align([item[1]], item[2], use_ctc=use_ctc_loss))
            continue
        pending.append(item)
        if len(pending) == group:
            flush(pending)
            pending = []
    flush(pending)
    return maes


def evaluate_batches(model, batches: Sequence[Any], lut: Optional[PinyinClassLUT] = None, use_ctc_loss: bool = False,
                     two_step: bool = False, rank: int = 0, world: int = 1, group: int = 1):
    """batches: sequence of (audios, tokens, _, lyric_word_onset_offset, _, _) as the reference's DataLoader yields.
    Returns (avg_mae, per_batch_maes) with skipped batches as None; identical on every rank.
    group (addition; default 1 = one device call per batch): `group` consecutive ONE-clip batches (the reference's default
    --batch-size 1) share one device call through AlignModel.align(per_clip=True); per-batch MAEs, skipped batches and the mean of
    per-batch means are those of group = 1.  A batch of more than one clip with group > 1 is a ValueError; so are two_step and
    world > 1 (the grouped path is the fused, single-rank one)."""
    if int(group) < 1:
        raise ValueError("evaluate_batches: group must be >= 1")
    if int(group) > 1:
        if two_step or world != 1:
            raise ValueError("evaluate_batches: group > 1 goes with two_step=False and world=1")
        with torch.no_grad():
            maes = _evaluate_grouped(model, batches, lut, use_ctc_loss, int(group))
        done = [m for m in maes if m is not None]
        total = 0
        for m in done:
            total += m
        return (total / len(done) if done else float("nan")), maes

    def run(i: int):
        audios, tokens, _, onset_offset, _, _ = batches[i]
        labels = lut(tokens) if lut is not None else torch.as_tensor(tokens)
        if onset_offset == (None,):
            return None
        if two_step:
            logits, _ = model.frame_manual_forward(audios)
            res = (perform_viterbi_ctc if use_ctc_loss else perform_viterbi)(logits, labels)
        else:
            res = model.align(audios, labels, use_ctc=use_ctc_loss)
        return get_mae(onset_offset, res)

    with torch.no_grad():
        maes = map_sharded(run, len(batches), rank, world)
    done = [m for m in maes if m is not None]
    total = 0
    for m in done:          # same accumulation order as the reference's running sum
        total += m
    avg = total / len(done) if done else float("nan")
    return avg, maes


def _align_records_batched(model, records: List[Any], lut, tokenize, use_ctc_loss: bool, with_confidence: bool, batch_size: int,
                           min_duration=None) -> List[list]:
    """align_records with records of at most 30 s sorted by length and aligned `batch_size` at a time (per_clip=True: each as if alone);
    results in the caller's order.  Longer records go one at a time through the dense long-form call."""
    out: List[Optional[list]] = [None] * len(records)
    short = sorted((i for i, r in enumerate(records) if len(r.audio) <= PER_CLIP_MAX_SAMPLES), key=lambda i: len(records[i].audio))
    for i, rec in enumerate(records):
        if len(rec.audio) > PER_CLIP_MAX_SAMPLES:
            out[i] = align_records(model, [rec], lut, tokenize, use_ctc_loss, with_confidence, min_duration=min_duration)[0]
    for k in range(0, len(short), batch_size):
        idx = short[k: k + batch_size]
        labels = [[int(v) for v in lut(torch.tensor([tokenize(records[i].text)], dtype=torch.long))[0].tolist()] for i in idx]
        audios = [records[i].audio for i in idx]
        if with_confidence:
            res, scores = model.align(audios, labels, use_ctc=use_ctc_loss, return_confidence=True, per_clip=True)
        else:
            res, scores = model.align(audios, labels, use_ctc=use_ctc_loss, per_clip=True, **_floor_kw(min_duration)), None
        for j, i in enumerate(idx):
            text = records[i].text
            if with_confidence:
                out[i] = [[res[j][n][0], res[j][n][1], text[n], scores[j]["occupancy"][n]] for n in range(len(res[j]))]
            else:
                out[i] = [[res[j][n][0], res[j][n][1], text[n]] for n in range(len(res[j]))]
    return out


def _floor_kw(min_duration) -> dict:
    """AlignModel.align's min_duration keyword where a floor is given; nothing otherwise (the call as it was)."""
    return {} if min_duration is None else {"min_duration": min_duration}


def align_records(model, records: Iterable[Any], lut: PinyinClassLUT, tokenize, use_ctc_loss: bool = True,
                  with_confidence: bool = False, batch_size: int = 1, min_duration=None) -> List[list]:
    """inference_alignment_nogt.py:130-178: one record at a time, returns [[onset, offset, char], ...] per record.
    `tokenize(text) -> list[int]` are the BERT ids without [CLS]/[SEP] (the reference slices [1:-1], :158-163).
    with_confidence (addition): each entry is [onset, offset, char, occupancy] (AlignModel.align(return_confidence=True)).
    batch_size (addition; default 1 = one record per device call, as the reference): records of at most 30 s are sorted by length and
    aligned batch_size at a time with AlignModel.align(per_clip=True) -- every record's result is the one it gets alone -- and returned
    in the caller's order; longer records go one at a time.
    min_duration (addition; None: the call as it was): one number of seconds, the least duration of every character
    (AlignModel.align(min_duration=...), at most 8 frames; it has not been tuned on real singing).  Not with with_confidence
    (ValueError: that lattice has no posteriors yet)."""
    if int(batch_size) < 1:
        raise ValueError("align_records: batch_size must be >= 1")
    if min_duration is not None and with_confidence:
        raise ValueError("align_records: min_duration does not go with with_confidence (no posteriors on the lattice with a minimum duration)")
    if int(batch_size) > 1:
        with torch.no_grad():
            return _align_records_batched(model, list(records), lut, tokenize, use_ctc_loss, with_confidence, int(batch_size), min_duration)
    out = []
    with torch.no_grad():
        for rec in records:
            ids = torch.tensor([tokenize(rec.text)], dtype=torch.long)
            if with_confidence:
                res, scores = model.align([rec.audio], lut(ids), use_ctc=use_ctc_loss, return_confidence=True)
                res, occ = res[0], scores[0]["occupancy"]
                out.append([[res[j][0], res[j][1], rec.text[j], occ[j]] for j in range(len(res))])
                continue
            res = model.align([rec.audio], lut(ids), use_ctc=use_ctc_loss, **_floor_kw(min_duration))[0]
            out.append([[res[j][0], res[j][1], rec.text[j]] for j in range(len(res))])
    return out


def _sheet_inputs(who: str, lines: Sequence[str], optional: Sequence[bool], lut: PinyinClassLUT, tokenize):
    """What the sheet functions hand to AlignModel.align: -> (token ids per line, optional_spans of the one clip, class-id labels [1, L])."""
    from .utils.alignment import spans_from_lines
    ids = [list(tokenize(line)) for line in lines]
    for line, tok in zip(lines, ids):
        if len(tok) != len(line):
            raise ValueError(f"{who}: {len(tok)} tokens for the {len(line)} characters of {line!r}")
    skip_from = spans_from_lines([len(t) for t in ids], optional)
    spans = [(a, n) for n, a in enumerate(skip_from) if a >= 0]
    labels = lut(torch.tensor([[v for tok in ids for v in tok]], dtype=torch.long))
    return ids, spans, labels


def _line_anchors(starts: Sequence[float], ids, tolerance_s: float) -> list:
    """One onset anchor per line: (index of the line's first character, the line's start time, tolerance_s)."""
    anchors, pos = [], 0
    for start, tok in zip(starts, ids):
        anchors.append((pos, start, float(tolerance_s)))
        pos += len(tok)
    return anchors


class _SheetKw(dict):
    """_reading_kw's keywords; _align_sheet leaves the clip's pronunciation scores here (None: not asked for), and with off-sheet slots
    the clip's slot visits and, where the call had a confidence that reports it, its off_sheet_prob dict."""
    pronunciation = None
    off_sheet = None
    off_sheet_prob = None
    line_of_position = None


def _reading_kw(lut: PinyinClassLUT, ids, heteronyms, with_pronunciation: bool = False, top_k: int = 5, off_sheet=False,
                off_sheet_penalty: float = math.log(100), who: str = "align") -> dict:
    """The keywords the sheet functions add to AlignModel.align for heteronyms (None: none): the alternatives of the one clip and
    return_readings, so that every character entry can name the class that was sung; with_pronunciation: the three keywords of the
    pronunciation scores, with every class of the lookup table (ids from 1) as a candidate; off_sheet (False: none; True: a slot before
    every line and one after the last; or a list of line indices, len(lines) = after the last line): the three keywords of the off-sheet
    slots, a slot in front of each such line's first character."""
    kw = _SheetKw()
    if off_sheet is not False and off_sheet is not None:
        starts = [0]
        for tok in ids:
            starts.append(starts[-1] + len(tok))
        before = list(range(len(starts))) if off_sheet is True else list(off_sheet)
        if any(isinstance(i, bool) or int(i) != i or not 0 <= int(i) < len(starts) for i in before) or len(set(before)) != len(before):
            raise ValueError(f"{who}: off_sheet: True, False or distinct line indices in 0..{len(ids)} ({len(ids)} = after the last line) expected")
        kw.line_of_position = {starts[int(i)]: int(i) for i in before}
        if before:
            kw.update(off_sheet=[sorted(kw.line_of_position)], off_sheet_penalty=off_sheet_penalty, return_off_sheet=True)
    if heteronyms is not None:
        kw.update(alternatives=lut.readings_of(torch.tensor([[v for tok in ids for v in tok]], dtype=torch.long), heteronyms), return_readings=True)
    if with_pronunciation:
        kw.update(return_pronunciation=True, pronunciation_classes=sorted(c for c in lut.syllables if c >= 1), pronunciation_top_k=top_k)
    return kw


def _align_sheet(model, reading_kw: dict, audio, labels, **kw):
    """model.align on the one clip with _reading_kw's keywords -> (what the call returns without them, the clip's readings or None); the
    clip's pronunciation scores, where asked for, are left in reading_kw.pronunciation."""
    out = model.align([audio], labels, **kw, **reading_kw)
    if not reading_kw:
        return out, None
    rest, readings = list(out), None
    if "return_off_sheet" in reading_kw:
        reading_kw.off_sheet = rest.pop()[0]
    if "return_pronunciation" in reading_kw:
        reading_kw.pronunciation = rest.pop()[0]
    if "return_readings" in reading_kw:
        readings = rest.pop()[0]
    if "return_off_sheet" in reading_kw and len(rest) > 1 and isinstance(rest[-1][0], dict):
        reading_kw.off_sheet_prob = rest[-1][0].get("off_sheet_prob")          # what is left: seconds [, segments] [, scores]
    return (rest[0] if len(rest) == 1 else tuple(rest)), readings


def _pronunciation_lines(pronunciation, lines: Sequence[str], lut: PinyinClassLUT) -> List[list]:
    """One clip's AlignModel.align(return_pronunciation=True) list -> one list per line with, per character, None (left out) or the dict
    with the character and syllable names added: {"char", "class", "syllable", "frames", "log_prob", "rank", "gop", "top": [(syllable,
    score per frame), ...]}."""
    out, pos = [], 0
    for line in lines:
        out.append([None if d is None else {"char": line[j], "class": d["class"], "syllable": lut.syllable_of(d["class"]), "frames": d["frames"],
                                            "log_prob": d["log_prob"], "rank": d["rank"], "gop": d["gop"],
                                            "top": [(lut.syllable_of(c), v) for c, v in d["top"]]}
                    for j, d in enumerate(pronunciation[pos: pos + len(line)])])
        pos += len(line)
    return out


def _done(result, reading_kw, lines: Sequence[str], lut: PinyinClassLUT):
    """What a sheet function returns: its result, or (result, pronunciation per line) where the pronunciation scores were asked for; with
    off-sheet slots the tuple gains the passages [(before_line, onset_s, offset_s[, [(syllable heard, score per frame), ...]]), ...] in time
    order and, where the call had a confidence, {before_line: off_sheet_prob} for every slot."""
    out = (result,)
    if getattr(reading_kw, "pronunciation", None) is not None:
        out += (_pronunciation_lines(reading_kw.pronunciation, lines, lut),)
    if getattr(reading_kw, "off_sheet", None) is not None:
        line_of = reading_kw.line_of_position
        out += ([(line_of[v["position"]], v["onset"], v["offset"]) + (([(lut.syllable_of(c), s) for c, s in v["top"]],) if "top" in v else ())
                 for v in reading_kw.off_sheet],)
        if reading_kw.off_sheet_prob is not None:
            out += ({line_of[n]: float(p) for n, p in reading_kw.off_sheet_prob.items()},)
    return out[0] if len(out) == 1 else out


def suspect_characters(result, max_rank: int = 0, min_gop: Optional[float] = None) -> List[tuple]:
    """The characters a proof-reader of the sheet would look at: result = the per-line pronunciation list that align_record_lines /
    align_record_lrc / align_song return with with_pronunciation=True -> [(line index, character index in the line, the syllable heard
    best there, gop), ...] for every sung character whose own class ranks behind max_rank candidates (rank > max_rank) or, where min_gop is
    given, whose gop lies below it.  min_gop is the caller's choice: no threshold has been measured on real singing, so none is built in
    (None: the rank alone decides)."""
    out = []
    for i, line in enumerate(result):
        for j, d in enumerate(line):
            if d is not None and (d["rank"] > max_rank or (min_gop is not None and d["gop"] < min_gop)):
                out.append((i, j, d["top"][0][0], d["gop"]))
    return out


def _align_repeat_sheet(model, reading_kw: dict, audio, labels, ids, spans, repeatable, use_ctc_loss, skip_penalty, repeat_penalty, **kw):
    """_align_sheet on the lattice where the lines with repeatable[i] may be sung again (repeat_spans from the flags: repeats_from_lines),
    with every visit as segments; kw: the confidence keyword and the anchors, if any."""
    from .utils.alignment import repeats_from_lines
    repeat_from = repeats_from_lines([len(t) for t in ids], repeatable)
    with torch.no_grad():
        return _align_sheet(model, reading_kw, audio, labels, use_ctc=use_ctc_loss, optional_spans=[spans], skip_penalty=skip_penalty,
                            repeat_spans=[[(a, e) for a, e in enumerate(repeat_from) if e >= 0]], repeat_penalty=repeat_penalty,
                            return_segments=True, **kw)


def _sheet_lines_out(res, lines: Sequence[str], per_line=(), readings=None):
    """One clip's per-character result -> one entry per line (None for a line left out: a span is taken or left as a whole, its characters
    are None together), and for every f of per_line the list of f(position of the line's first character, its result).  readings (the
    clip's, AlignModel.align(return_readings=True)): every character entry gains the class id that was sung."""
    out: List[Optional[list]] = []
    extra = [[] for _ in per_line]
    pos = 0
    for line in lines:
        part = res[pos: pos + len(line)]
        for values, f in zip(extra, per_line):
            values.append(f(pos, part[0]))
        out.append(None if part[0] is None else
                   [[part[j][0], part[j][1], line[j]] + ([] if readings is None else [readings[pos + j][0]]) for j in range(len(line))])
        pos += len(line)
    return (out, *extra)


def _line_occurrences(segments, lines: Sequence[str], readings=None) -> List[list]:
    """One clip's visits (char_index, onset_s, offset_s) in time order -> per line the list of its occurrences, each [[onset, offset, char],
    ...]: a new occurrence of a line begins where a visit does not continue the line's last one (its character index does not go up)."""
    out: List[list] = [[] for _ in lines]
    for (n, on, off), (i, k, j) in zip(segments, _occurrence_of_visits(segments, lines)):
        if k == len(out[i]):
            out[i].append([])
        out[i][k].append([on, off, lines[i][j]] + ([] if readings is None else [readings[n][0]]))
    return out


def _occurrence_of_visits(segments, lines: Sequence[str]) -> List[tuple]:
    """Per visit of _line_occurrences' input: (its line, which occurrence of that line it belongs to, its character's index in the line)."""
    start_of, line_of = [], []
    for i, line in enumerate(lines):
        start_of.append(len(line_of))
        line_of += [i] * len(line)
    count = [0] * len(lines)
    out, last = [], None                         # last: (line, character index) of the previous visit
    for n, _, _ in segments:
        i = line_of[n]
        if last is None or last[0] != i or n <= last[1]:
            count[i] += 1
        out.append((i, count[i] - 1, n - start_of[i]))
        last = (i, n)
    return out


def _timed_lines(who: str, lrc) -> List[tuple]:
    pairs = parse_lrc(lrc) if isinstance(lrc, str) else [(float(s), str(line)) for s, line in lrc]
    if not pairs:
        raise ValueError(f"{who}: no timed line in the sheet")
    return pairs


def _sheet_confidence(res, scores, lines: Sequence[str], readings=None):
    """-> (lines_out, conf) of align_record_lrc(with_confidence=True) from one clip's seconds and its anchored / sheet score dict."""
    out, sung, line_onset = _sheet_lines_out(res, lines, (lambda pos, first: float(scores["sung_prob"][pos]),
                                                          lambda pos, first: None if first is None else float(scores["onset_prob"][pos])),
                                                  readings)
    return out, {"sung": sung, "line_onset_prob": line_onset, "window_log_prob": float(scores["window_log_prob"])}


def _visit_confidence(segments, scores, lines: Sequence[str], ids, repeatable, readings=None):
    """-> (occurrences, conf) of align_record_lines(with_visit_confidence=True) from one clip's visits and its repeat / song score dict."""
    occurrences = _line_occurrences(segments, lines, readings)
    per = [[[] for _ in occ] for occ in occurrences]
    for v, (i, k, _) in zip(scores["visit_occupancy"], _occurrence_of_visits(segments, lines)):
        per[i][k].append(v)
    conf, pos = [], 0
    for i, line in enumerate(lines):
        conf.append({"visits": float(scores["visits"][pos]),
                     "repeat_count": scores["repeat_count"].get((pos, pos + len(ids[i]))) if repeatable[i] else None,
                     "occurrence_occupancy": [float(np.mean(v)) for v in per[i]]})
        pos += len(ids[i])
    return occurrences, conf


def align_record_lines(model, audio, lines: Sequence[str], optional: Sequence[bool], lut: PinyinClassLUT, tokenize,
                       use_ctc_loss: bool = True, skip_penalty: float = 0.0, with_confidence: bool = False, repeatable=None,
                       repeat_penalty: float = 0.0, with_visit_confidence: bool = False, heteronyms=None, with_pronunciation: bool = False,
                       top_k: int = 5, off_sheet=False, off_sheet_penalty: float = math.log(100), min_duration=None):
    """One recording against a lyric sheet given line by line (addition; the reference aligns exactly what is sung): lines with
    optional[i] may be absent from the audio (a chorus printed once more than sung, a bracketed ad-lib).  `tokenize(line)` as in
    align_records, one class per character.  -> one entry per line: None if the alignment left the line out, otherwise
    [[onset, offset, char], ...] (AlignModel.align(optional_spans=...), skip_penalty >= 0 per skipped line).
    with_confidence: -> (lines_out, sung), sung[i] = the probability under the model that line i was sung (a Python float: present_prob
    of the line's first character, AlignModel.align(return_span_confidence=True)); 1 for a mandatory line, and 1 - span_skip_prob of an
    optional line's span.
    Up to 4095 characters in the sheet; with_confidence at most 511 (NotImplementedError; align_song gives the confidences of a whole song).
    repeatable (one flag per line; None: the result as above): lines with repeatable[i] may be sung again right after they were sung (a
    chorus marked "x2"; AlignModel.align(repeat_spans=...), repeat_penalty >= 0 per return).  Each line's entry is then the LIST of its
    occurrences in time order, each [[onset, offset, char], ...] -- empty if the alignment left the line out.  Not with with_confidence
    (ValueError).
    with_visit_confidence (with repeatable; at most 511 characters -- align_song(repeatable=...) takes whole songs): -> (occurrences, conf), conf[i] = {"visits": the expected number of
    times line i was sung (AlignModel.align(return_repeat_confidence=True)'s `visits` of its first character: an expected count, it can
    exceed 1), "repeat_count": the expected number of returns of a repeatable line (None for the others), "occurrence_occupancy": one
    number per listed occurrence, the mean visit_occupancy of its characters}.
    heteronyms (here, in align_record_lrc and in align_song; None: the outputs as above): {token id: [syllable, ...]}, the further syllables
    a character may be sung as (PinyinClassLUT.readings_of; AlignModel.align(alternatives=..., return_readings=True)).  Every character
    entry is then [onset, offset, char, class_id_sung].
    with_pronunciation / top_k (here, in align_record_lrc and in align_song; off: the outputs as above): was the sheet's character the one
    that was sung?  -> (the result as above, pronunciation): one list per line with, per character, None (left out) or {"char", "class",
    "syllable", "frames", "log_prob", "rank", "gop", "top": [(syllable, score per frame), ... top_k of them]} -- AlignModel.align(
    return_pronunciation=True) with every class of the lookup table as a candidate; rank 0 = the sheet's syllable scored best over the
    character's segment, gop <= 0 its per-frame distance to the best.  suspect_characters picks the entries worth a look.
    off_sheet / off_sheet_penalty (here, in align_record_lrc and in align_song; False: the outputs as above): singing that is not on the
    sheet -- ad-libs between lines, backing vocals, an omitted verse.  True puts a slot before every line and one after the last; a list
    names the lines to put one in front of (len(lines) = after the last line); AlignModel.align(off_sheet=..., return_off_sheet=True).
    The return gains the passages as its last element: [(before_line, onset_s, offset_s), ...] in time order, one per slot that was used
    (with with_pronunciation each also holds [(syllable heard, score per frame), ...]); with a confidence option one more element,
    {before_line: off_sheet_prob}, the probability that the slot was used at all.  off_sheet_penalty (nats per frame, default ln 100: a
    character must hold less than 1 % of the voiced probability to lose a frame to a slot) has not been tuned on real singing; keep it
    above skip_penalty.
    min_duration (None: the outputs as above): one number of seconds, the least duration of every character
    (AlignModel.align(min_duration=...), at most 8 frames; not tuned on real singing).  The floor exists on the plain lattice alone:
    ValueError together with an optional line, with_confidence, repeatable, with_visit_confidence or off_sheet; with heteronyms and
    with_pronunciation."""
    lines = list(lines)
    if min_duration is not None:
        for name, given in (("optional", any(bool(v) for v in optional)), ("with_confidence", with_confidence), ("repeatable", repeatable is not None),
                            ("with_visit_confidence", with_visit_confidence), ("off_sheet", off_sheet is not False and off_sheet is not None)):
            if given:
                raise ValueError(f"align_record_lines: min_duration does not go with {name} (the floor exists on the plain lattice alone)")
    ids, spans, labels = _sheet_inputs("align_record_lines", lines, optional, lut, tokenize)
    rk = _reading_kw(lut, ids, heteronyms, with_pronunciation, top_k, off_sheet, off_sheet_penalty, "align_record_lines")
    if with_visit_confidence and repeatable is None:
        raise ValueError("align_record_lines: with_visit_confidence goes with repeatable (with_confidence is the keyword without it)")
    if repeatable is not None:
        if with_confidence:
            raise ValueError("align_record_lines: repeatable does not go with with_confidence (no posteriors on the lattice with repeatable spans)")
        sheet = (model, rk, audio, labels, ids, spans, repeatable, use_ctc_loss, skip_penalty, repeat_penalty)
        if with_visit_confidence:
            (_, segments, scores), readings = _align_repeat_sheet(*sheet, return_repeat_confidence=True)
            return _done(_visit_confidence(segments[0], scores[0], lines, ids, repeatable, readings), rk, lines, lut)
        (_, segments), readings = _align_repeat_sheet(*sheet)
        return _done(_line_occurrences(segments[0], lines, readings), rk, lines, lut)
    with torch.no_grad():
        if with_confidence:
            (res, scores), readings = _align_sheet(model, rk, audio, labels, use_ctc=use_ctc_loss, optional_spans=[spans],
                                                   skip_penalty=skip_penalty, return_span_confidence=True)
            present = scores[0]["sung_prob"]
            return _done(_sheet_lines_out(res[0], lines, (lambda pos, first: float(present[pos]),), readings), rk, lines, lut)
        res, readings = _align_sheet(model, rk, audio, labels, use_ctc=use_ctc_loss, optional_spans=[spans], skip_penalty=skip_penalty,
                                     **_floor_kw(min_duration))
    return _done(_sheet_lines_out(res[0], lines, (), readings)[0], rk, lines, lut)


def align_free_order(model, audio, lines: Sequence[str], lut: PinyinClassLUT, tokenize, use_ctc_loss: bool = True,
                     line_jump_penalty: float = 0.0, heteronyms=None) -> dict:
    """One recording against an UNMARKED lyric sheet (addition): the sheet as found prints each verse and the chorus once, in print
    order; the song sings them in its own order, some of them again, some not at all, and an excerpt starts and ends where it likes.
    Nothing is marked -- no optional flag, no "x2", no slot: the line breaks are all the lattice is given
    (AlignModel.align(line_starts=..., return_segments=True); line_jump_penalty >= 0 per change of line that the sheet's own order does
    not give, per start at another line than the first and per end at another than the last).  The default 0.0 follows skip_penalty /
    repeat_penalty and HAS NOT BEEN TUNED on real singing.  `tokenize(line)` as in align_records, one class per character; up to 4095
    characters in the sheet.
    -> {"occurrences": per line the time-ordered list of its occurrences, each [[onset, offset, char], ...] (empty for a line never
    sung), "order": the line index of every occurrence in time order, e.g. [1, 0, 1, 2, 1], "unsung": the indices of the lines never
    sung}.  heteronyms (None: the entries as above): as in align_record_lines; every character entry is then [onset, offset, char,
    class_id_sung], the class read off the character's first visit."""
    return _free_order("align_free_order", model, audio, lines, lut, tokenize, use_ctc_loss, line_jump_penalty, heteronyms)


def _free_order(who: str, model, audio, lines, lut, tokenize, use_ctc_loss, line_jump_penalty, heteronyms, boundary_window=None) -> dict:
    """align_free_order's dict; with a boundary_window the call also asks for the line confidence and the dict gains "confidence"."""
    lines = list(lines)
    ids, _, labels = _sheet_inputs(who, lines, [False] * len(lines), lut, tokenize)
    starts, pos = [], 0
    for tok in ids:
        starts.append(pos)
        pos += len(tok)
    rk = _reading_kw(lut, ids, heteronyms, who=who)
    kw = {} if boundary_window is None else dict(return_line_confidence=True, boundary_window=int(boundary_window))
    with torch.no_grad():
        res, readings = _align_sheet(model, rk, audio, labels, use_ctc=use_ctc_loss, line_starts=[starts],
                                     line_jump_penalty=line_jump_penalty, return_segments=True, **kw)
    segments = res[1]
    occurrences = _line_occurrences(segments[0], lines, readings)
    visits = _occurrence_of_visits(segments[0], lines)
    order, last = [], None
    for i, k, _ in visits:
        if (i, k) != last:
            order.append(i)
        last = (i, k)
    out = {"occurrences": occurrences, "order": order, "unsung": [i for i, occ in enumerate(occurrences) if not occ]}
    if boundary_window is not None:
        d = res[2][0]
        weight = [[[0.0, 0.0] for _ in occ] for occ in occurrences]          # per occurrence: posterior times seconds, seconds
        for (n, on, off), (i, k, _), v in zip(segments[0], visits, d["visit_occupancy"]):
            weight[i][k][0] += v * (off - on)
            weight[i][k][1] += off - on
        out["confidence"] = {"expected_occurrences": list(d["line_visits"]), "out_of_order": list(d["line_out_of_order"]),
                             "occurrence_occupancy": [[a / b for a, b in occ] for occ in weight],
                             "order_log_posterior": d["path_log_posterior"]}
    return out


def align_free_order_scored(model, audio, lines: Sequence[str], lut: PinyinClassLUT, tokenize, use_ctc_loss: bool = True,
                            line_jump_penalty: float = 0.0, heteronyms=None, boundary_window: int = 2) -> dict:
    """align_free_order plus how far to trust it (addition): the same dict and "confidence", from the posteriors of the lattice with free
    line order (AlignModel.align(line_starts=..., return_line_confidence=True)):
      "expected_occurrences": per line the expected number of times it is sung under the model -- a COUNT, not a probability: a chorus
          sung three times is near 3, a line left out near 0, and a line the model cannot place may sit anywhere between;
      "out_of_order": per line how many of those occurrences are expected to begin out of print order (by a jump or a free start);
      "occurrence_occupancy": per line one number per reported occurrence, the mean posterior of the reported state over the frames of
          the occurrence's characters (near 1: the model puts these frames nowhere else);
      "order_log_posterior": final_score - log_z <= 0, the log-probability of the reported order and timing together.
    line_jump_penalty (default 0.0) has not been tuned on real singing; these numbers are the means to tune it."""
    return _free_order("align_free_order_scored", model, audio, lines, lut, tokenize, use_ctc_loss, line_jump_penalty, heteronyms,
                       boundary_window)


_LRC_TAG = re.compile(r"\[([^\[\]]*)\]")
_LRC_TIME = re.compile(r"^(\d+):(\d{1,2})(?:[.:](\d{1,3}))?$")


def parse_lrc(text: str) -> List[tuple]:
    """LRC lyric sheet -> [(start_seconds, line), ...] sorted by time (a stable sort: equal times keep the file's order).  Time tags are
    [mm:ss], [mm:ss.xx] and [mm:ss.xxx]; several tags in front of one line repeat the line; metadata tags ([ar:...], [ti:...], [offset:...])
    and lines without text are dropped."""
    out = []
    for raw in str(text).splitlines():
        rest, times = raw.strip(), []
        while True:
            m = _LRC_TAG.match(rest)
            if m is None:
                break
            t = _LRC_TIME.match(m.group(1).strip())
            if t is not None:
                frac = t.group(3) or ""
                times.append(60.0 * int(t.group(1)) + int(t.group(2)) + (int(frac) / 10.0 ** len(frac) if frac else 0.0))
            rest = rest[m.end():].lstrip()
        if rest and times:
            out += [(s, rest) for s in times]
    out.sort(key=lambda v: v[0])
    return out


def align_record_lrc(model, audio, lrc, lut: PinyinClassLUT, tokenize, tolerance_s: float = 1.0, optional: Optional[Sequence[bool]] = None,
                     use_ctc_loss: bool = True, skip_penalty: float = 0.0, with_confidence: bool = False, heteronyms=None,
                     with_pronunciation: bool = False, top_k: int = 5, off_sheet=False, off_sheet_penalty: float = math.log(100)):
    """One recording against an LRC sheet (addition): per-character timing from per-line start times.  `lrc` is LRC text (parse_lrc) or a
    list of (start_seconds, line) pairs; the first character of every line gets an onset anchor at the line's start time with tolerance_s
    (AlignModel.align(onset_anchors=...): the line starts within tolerance_s of its tag, and everything before it has ended by then).
    optional[i] marks lines that may be absent, as in align_record_lines (default: none).  `tokenize(line)` as in align_records, one class per
    character.  -> one entry per line: None for a line the alignment left out, otherwise [[onset, offset, char], ...].  ValueError when no
    path lies inside the anchors' windows (a tag further from its line than tolerance_s).
    with_confidence: -> (lines_out, conf) with the posteriors GIVEN the tags (AlignModel.align(return_anchored_confidence=True)):
    conf = {"sung": [per line, as align_record_lines: the probability that the line was sung, 1 for a mandatory line],
            "line_onset_prob": [per line: the probability that the line's first character starts within boundary_window = 2 frames of
                                the reported onset, None for a line that was left out],
            "window_log_prob": float <= 0, the log-probability the unanchored model gives to "the path respects every tag" -- near 0
                               when the sheet agrees with the audio, strongly negative when a tag is off by more than tolerance_s}.
    Up to 4095 characters in the sheet; with_confidence at most 511 (NotImplementedError; align_song gives the confidences of a whole song).
    heteronyms: as in align_record_lines -- every character entry becomes [onset, offset, char, class_id_sung].
    with_pronunciation / top_k: as in align_record_lines -- -> (the result as above, pronunciation per line).
    off_sheet / off_sheet_penalty: as in align_record_lines -- the return gains the passages and, with with_confidence, off_sheet_prob."""
    pairs = _timed_lines("align_record_lrc", lrc)
    lines = [line for _, line in pairs]
    optional = [False] * len(lines) if optional is None else list(optional)
    ids, spans, labels = _sheet_inputs("align_record_lrc", lines, optional, lut, tokenize)
    anchors = _line_anchors([start for start, _ in pairs], ids, tolerance_s)
    rk = _reading_kw(lut, ids, heteronyms, with_pronunciation, top_k, off_sheet, off_sheet_penalty, "align_record_lrc")
    with torch.no_grad():
        if with_confidence:
            (res, scores), readings = _align_sheet(model, rk, audio, labels, use_ctc=use_ctc_loss, optional_spans=[spans],
                                                   skip_penalty=skip_penalty, onset_anchors=[anchors], return_anchored_confidence=True)
            return _done(_sheet_confidence(res[0], scores[0], lines, readings), rk, lines, lut)
        res, readings = _align_sheet(model, rk, audio, labels, use_ctc=use_ctc_loss, optional_spans=[spans], skip_penalty=skip_penalty,
                                     onset_anchors=[anchors])
    return _done(_sheet_lines_out(res[0], lines, (), readings)[0], rk, lines, lut)


def align_song(model, audio, sheet, lut: PinyinClassLUT, tokenize, tolerance_s: float = 1.0, optional: Optional[Sequence[bool]] = None,
               use_ctc_loss: bool = True, skip_penalty: float = 0.0, repeatable: Optional[Sequence[bool]] = None, repeat_penalty: float = 0.0,
               heteronyms=None, with_pronunciation: bool = False, top_k: int = 5, off_sheet=False, off_sheet_penalty: float = math.log(100)):
    """A whole song against its whole sheet, timing and confidences in one call (addition): up to 4095 characters.  `sheet` is LRC text
    (parse_lrc), a list of (start_seconds, line) pairs -- every line's first character anchored at its start time with tolerance_s, as in
    align_record_lrc -- or a list of plain lines (no times: no anchors, as in align_record_lines).  optional[i] marks lines that may be
    absent from the audio (default: none).  -> (lines_out, conf) in align_record_lrc(with_confidence=True)'s form, from
    AlignModel.align(return_sheet_confidence=True): lines_out has one entry per line (None for a line left out), conf = {"sung": [per line],
    "line_onset_prob": [per line, None for a line left out], "window_log_prob": float <= 0 (0.0 for a sheet without times)}.  Up to 511
    characters the numbers are align_record_lrc's exactly.  The posterior sweep keeps every alpha row on the device: frames * 1024 R * 8
    bytes beyond 511 characters (R = 2 / 4 / 8 for up to 1023 / 2047 / 4095): 197 MB for a four-minute song of 800 characters.
    repeatable (one flag per line; None: the call and its result as above): lines with repeatable[i] may be sung again right after they
    were sung (a chorus printed once and marked "x2"; repeat_penalty >= 0 per return), as in align_record_lines(repeatable=...);
    AlignModel.align(repeat_spans=..., return_song_confidence=True).  Each entry of lines_out is then the LIST of that line's occurrences
    in time order, each [[onset, offset, char], ...] -- empty for a line left out.  conf keeps "sung" (the probability that the line was
    sung at all: the expected visits of its first character that are not returns, visits - repeat_count), "line_onset_prob" (about the
    first occurrence; None for a line left out) and "window_log_prob", and gains "visits", "repeat_count" and "occurrence_occupancy",
    one value per line as align_record_lines(with_visit_confidence=True) defines them.  ValueError unless one flag per line.
    heteronyms: as in align_record_lines -- every character entry becomes [onset, offset, char, class_id_sung], and the confidences are
    posteriors of the merged classes.
    with_pronunciation / top_k: as in align_record_lines -- -> ((lines_out, conf), pronunciation per line).
    off_sheet / off_sheet_penalty: as in align_record_lines -- the return gains the passages and {before_line: off_sheet_prob}; a partial
    sheet (only the chorus) against a whole song is off_sheet=True."""
    if isinstance(sheet, str) or (len(sheet) > 0 and not isinstance(sheet[0], str)):
        pairs = _timed_lines("align_song", sheet)
        lines, starts = [line for _, line in pairs], [start for start, _ in pairs]
    else:
        lines, starts = [str(line) for line in sheet], None
        if not lines:
            raise ValueError("align_song: no line in the sheet")
    if repeatable is not None and len(repeatable) != len(lines):
        raise ValueError(f"align_song: {len(repeatable)} repeatable flags for {len(lines)} lines")
    optional = [False] * len(lines) if optional is None else list(optional)
    ids, spans, labels = _sheet_inputs("align_song", lines, optional, lut, tokenize)
    kw = {} if starts is None else {"onset_anchors": [_line_anchors(starts, ids, tolerance_s)]}
    rk = _reading_kw(lut, ids, heteronyms, with_pronunciation, top_k, off_sheet, off_sheet_penalty, "align_song")
    if repeatable is not None:
        (res, segments, scores), readings = _align_repeat_sheet(model, rk, audio, labels, ids, spans, repeatable, use_ctc_loss, skip_penalty,
                                                                repeat_penalty, return_song_confidence=True, **kw)
        occurrences, per_line = _visit_confidence(segments[0], scores[0], lines, ids, repeatable, readings)
        _, line_onset = _sheet_lines_out(res[0], lines, (lambda pos, first: None if first is None else float(scores[0]["onset_prob"][pos]),))
        conf = {"sung": [c["visits"] - (c["repeat_count"] or 0.0) for c in per_line], "line_onset_prob": line_onset,
                "window_log_prob": float(scores[0].get("window_log_prob", 0.0)),
                "visits": [c["visits"] for c in per_line], "repeat_count": [c["repeat_count"] for c in per_line],
                "occurrence_occupancy": [c["occurrence_occupancy"] for c in per_line]}
        return _done((occurrences, conf), rk, lines, lut)
    with torch.no_grad():
        (res, scores), readings = _align_sheet(model, rk, audio, labels, use_ctc=use_ctc_loss, optional_spans=[spans],
                                               skip_penalty=skip_penalty, return_sheet_confidence=True, **kw)
    return _done(_sheet_confidence(res[0], scores[0], lines, readings), rk, lines, lut)


def lrc_training_clips(audio, lrc, tokenize, max_seconds: float = 30.0, tolerance_s: float = 1.0, sample_rate: int = 16000) -> List[dict]:
    """One recording and its LRC sheet -> training clips for FineTuner.micro_step_anchored / utils.alignment.anchored_alignment_loss
    (addition; host only): [{"audio": samples of the clip, "lines": [line, ...], "onset_anchors": [(first character index of the line,
    tag - clip start in seconds, tolerance_s), ...]}, ...].  `lrc` is LRC text (parse_lrc) or a list of (start_seconds, line) pairs;
    `tokenize(line)` as in align_records, one class per character (used for the character counts).
    Consecutive lines are packed greedily: a clip starts tolerance_s before its first line's tag (not before 0) and ends where the next clip
    starts (the last one where the audio ends), capped at max_seconds; the next line joins a clip as long as the clip, ending where the line
    after it would start a clip of its own, stays within max_seconds.  A gap longer than max_seconds after a line therefore ends the clip at
    the cap, and the next clip starts tolerance_s before the next tag.  ValueError for a line that cannot fit: more characters than its clip
    has 20 ms frames, or a tag that lies at or behind the end of its clip (of the audio)."""
    pairs = parse_lrc(lrc) if isinstance(lrc, str) else sorted(((float(s), str(line)) for s, line in lrc), key=lambda v: v[0])
    if not pairs:
        raise ValueError("lrc_training_clips: no timed line in the sheet")
    max_seconds, tol = float(max_seconds), float(tolerance_s)
    if not max_seconds > 0.0 or tol < 0.0:
        raise ValueError("lrc_training_clips: max_seconds > 0 and tolerance_s >= 0 expected")
    total = len(audio) / float(sample_rate)
    counts = []
    for _, line in pairs:
        n = len(list(tokenize(line)))
        if n != len(line):
            raise ValueError(f"lrc_training_clips: {n} tokens for the {len(line)} characters of {line!r}")
        counts.append(n)
    own_start = [max(0.0, s - tol) for s, _ in pairs]       # where a clip that begins with line i starts

    def end_after(j, start):                                # end of a clip from `start` whose last line is j
        nxt = own_start[j + 1] if j + 1 < len(pairs) else total
        return min(nxt, total, start + max_seconds)

    clips = []
    i = 0
    while i < len(pairs):
        start = own_start[i]
        j = i
        while j + 1 < len(pairs) and (own_start[j + 2] if j + 2 < len(pairs) else total) <= start + max_seconds and pairs[j + 1][0] < total:
            j += 1
        end = end_after(j, start)
        frames = int((end - start) / 0.02 + 1e-9)
        anchors, pos = [], 0
        for k in range(i, j + 1):
            tag, line = pairs[k]
            if tag - start >= end - start:
                raise ValueError(f"lrc_training_clips: line {k} ({line!r}) is tagged at {tag:.2f} s, at or behind the end of its clip ({end:.2f} s)")
            anchors.append((pos, tag - start, tol))
            pos += counts[k]
        if pos > frames:
            raise ValueError(f"lrc_training_clips: lines {i}..{j} hold {pos} characters, their clip of {end - start:.2f} s only {frames} frames")
        clips.append({"audio": audio[int(round(start * sample_rate)): int(round(end * sample_rate))], "lines": [pairs[k][1] for k in range(i, j + 1)],
                      "onset_anchors": anchors})
        i = j + 1
    return clips
