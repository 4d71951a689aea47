"""Post-processing next to the hot path: the reference's ``median_filter``
(src/utils/helper.py:66-97) and the run-length interval extraction of ``get_new_cuts``
(src/scripts/predict.py:472-490).  The filter runs on the GPU (``uvad_median_filter``) instead of
the reference's device -> CPU -> scipy -> "cuda" round trip; the interval walk is vectorised.  The scoring side
(``supervision_frames``, ``score_metrics``, ``det_curve``) is the host half of ``uvad_score_*``."""
from typing import List, Tuple

import numpy as np
import torch


def median_window(window: float, speech_window: float = 0.5) -> int:
    """Tap count the reference derives: int(SPEECH_WINDOW / window), made odd (49 @ 10 ms, 25 @ 20 ms)."""
    k = int(speech_window / window)
    return k - 1 if k % 2 == 0 else k


def median_filter(x: torch.Tensor, SPEECH_WINDOW: float = 0.5, window: float = 0.02, runtime=None, lengths=None) -> torch.Tensor:
    """(batch, frames) probabilities -> (batch, frames) int64 0/1, same contract as the reference
    (which returns the tensor on "cuda"); thresholds at 0.5 then applies the odd binary median
    with zero-padded edges.  lengths (batch,): valid frames per row -- each row's prefix is filtered
    alone (zero padded at its own end), labels past it are 0."""
    if not x.is_cuda:
        raise RuntimeError("median_filter runs on the GPU only")
    if runtime is None:
        from .runtime import VadRuntime
        runtime = _shared_runtime(x.device)
    return runtime.median_filter(x, median_window(window, SPEECH_WINDOW), lengths=lengths).to(torch.int64)


def sliding_weights(kind: str, W: int) -> np.ndarray:
    """The aggregation weights (W,) f32 of the sliding calls (VadRuntime.sliding_configure): "rect" -- every window counts alike at every
    frame -- or "hamming", 0.54 - 0.46 cos(2 pi k / (W - 1)), which trusts a window's middle (the BiLSTM has context on both sides there)
    over its edges; its smallest value is 0.08, so every weight is > 0 as the library requires."""
    if W < 1:
        raise ValueError(f"W must be >= 1, got {W}")
    if kind == "rect" or W == 1:
        if kind not in ("rect", "hamming"):
            raise ValueError(f"unknown sliding weights {kind!r} (rect, hamming)")
        return np.ones(W, np.float32)
    if kind == "hamming":
        return (0.54 - 0.46 * np.cos(2.0 * np.pi * np.arange(W) / (W - 1))).astype(np.float32)
    raise ValueError(f"unknown sliding weights {kind!r} (rect, hamming)")


_RT = {}


def _shared_runtime(device):
    from .runtime import VadRuntime
    key = str(device)
    if key not in _RT:
        _RT[key] = VadRuntime(device=device, fbank=None, model=None)
    return _RT[key]


def labels_to_intervals(labels, frame_shift: float) -> List[Tuple[float, float]]:
    """One row of 0/1 frame labels -> [(start_s, end_s)], predict.py:472-490: a run that starts at
    frame k and whose first non-speech frame is k2 gives (round(k*shift, 2), round((k2-1)*shift, 2)),
    kept only if end - start > 0; a run still open at the end closes at (len-1)*shift."""
    v = np.asarray(labels.cpu() if torch.is_tensor(labels) else labels).astype(np.int8).ravel()
    if v.size == 0:
        return []
    d = np.diff(np.concatenate(([0], v, [0])))
    starts = np.flatnonzero(d == 1)
    stops = np.flatnonzero(d == -1)       # first non-speech frame after each run (== len for an open run)
    out = []
    for k, k2 in zip(starts, stops):
        last = (len(v) - 1) if k2 >= len(v) else (k2 - 1)
        s, e = round(float(k * frame_shift), 2), round(float(last * frame_shift), 2)
        if e - s > 0.0:
            out.append((s, e))
    return out


def labels_to_intervals_batch(labels: torch.Tensor, frame_shift: float, runtime=None, lengths=None) -> List[List[Tuple[float, float]]]:
    """(B, T) 0/1 labels ON THE GPU -> per row [(start_s, end_s)], same values as ``labels_to_intervals`` row by row.
    The run-length walk runs in ``uvad_label_runs``; only the (start, stop) frame pairs cross to the host (one copy
    for the whole batch), where the reference's rounding / empty-interval rule is applied.  lengths (B,): valid frames
    per row; row b gives what ``labels_to_intervals(labels[b, :lengths[b]])`` gives."""
    if not (torch.is_tensor(labels) and labels.is_cuda):
        raise RuntimeError("labels_to_intervals_batch runs on the GPU only (use labels_to_intervals for host rows)")
    if labels.dim() == 3:
        labels = labels.squeeze(-1)
    rt = runtime or _shared_runtime(labels.device)
    T = labels.shape[1]
    runs, counts = rt.label_runs(labels, lengths=lengths)
    if lengths is None:
        lens_h = [T] * labels.shape[0]
    else:   # the kernel clamped them to [0, T]; so does the host side
        lens_h = [min(max(int(v), 0), T) for v in (lengths.tolist() if torch.is_tensor(lengths) else lengths)]
    counts_h = counts.cpu().numpy()
    runs_h = runs[:, : max(int(counts_h.max()), 1)].cpu().numpy()
    out = []
    for b in range(labels.shape[0]):
        row = []
        Tb = lens_h[b]
        for k, k2 in runs_h[b, : counts_h[b]]:
            last = (Tb - 1) if k2 >= Tb else (k2 - 1)
            s, e = round(float(k * frame_shift), 2), round(float(last * frame_shift), 2)
            if e - s > 0.0:
                row.append((s, e))
        out.append(row)
    return out


# ---- SincNet (PyanNet) frames -> seconds, src/scripts/predict_sincnet.py:492-504 ----------------------------------
SINC_RF_1, SINC_RF_2 = 991, 1261           # receptive field of 1 and of 2 output frames (src/utils/receptive_field.py:197-215)
SINC_STEP = SINC_RF_2 - SINC_RF_1          # 270 samples between frame centres
SINC_HALF = round(0.5 * SINC_RF_1)         # the reference's comment says 495; its code, round(495.5), gives 496 (round-half-even) -- the code wins


def sincnet_frame_times(start: int, end: int, duration: float, sample_rate: int = 16000):
    """get_timestamp_from_sample_boundary (predict_sincnet.py:492-504): frame k of the SincNet front end is centred on sample
    k * 270 + 496 (SINC_HALF); the reference rounds that to WHOLE seconds (Python round), clamps the start at 0 and the end at the
    recording's duration."""
    s = round((start * SINC_STEP + SINC_HALF) / sample_rate)
    e = round((end * SINC_STEP + SINC_HALF) / sample_rate)
    return max(s, 0), min(e, duration)


def sincnet_labels_to_intervals(labels, duration: float, runtime=None) -> List[Tuple[float, float]]:
    """One recording's 0/1 frame labels (SincNet frame rate) -> [(start_s, end_s)] as get_new_cuts of predict_sincnet.py
    walks them (:348-370): a run of frames [k, k2) maps through sincnet_frame_times(k, k2 - 1, duration), kept only if
    end - start > 0.  Labels on the GPU go through uvad_label_runs; host rows are walked with numpy."""
    if torch.is_tensor(labels) and labels.is_cuda:
        rt = runtime or _shared_runtime(labels.device)
        runs, counts = rt.label_runs(labels.reshape(1, -1))
        n = int(counts.cpu()[0])
        pairs = runs[0, :n].cpu().numpy()
    else:
        v = np.asarray(labels.cpu() if torch.is_tensor(labels) else labels).astype(np.int8).ravel()
        d = np.diff(np.concatenate(([0], v, [0])))
        pairs = np.stack([np.flatnonzero(d == 1), np.flatnonzero(d == -1)], axis=1) if v.size else np.zeros((0, 2), np.int64)
    out = []
    for k, k2 in pairs:
        s, e = sincnet_frame_times(int(k), int(k2) - 1, duration)
        if e - s > 0.0:
            out.append((s, e))
    return out


# ---- scoring side of get_new_cuts (src/scripts/predict.py:500-509, 612-673) -----------------------------------

def merge_intervals_with_buffer(intervals, total_duration: float, buffer: float):
    """predict.py:614-634: widen every interval by `buffer` (clipped to the recording) and merge overlaps."""
    if len(intervals) == 0:
        return []
    iv = sorted(([max(s - buffer, 0), min(e + buffer, total_duration)] for s, e in intervals), key=lambda x: x[0])
    out = [list(iv[0])]
    for s, e in iv[1:]:
        if s <= out[-1][1]:
            out[-1][1] = e          # as the reference: the later interval's end replaces (not max) the running end
        else:
            out.append([s, e])
    return out


def merged_runs(labels, pad: int) -> List[Tuple[int, int]]:
    """merge_intervals_with_buffer in FRAMES on one row of 0/1 labels (host; what uvad_endpoint_step reports as events, restated): every run
    [s, c) becomes [max(s - pad, 0), min(c + pad, len)), and an interval merges into its predecessor when its start <= the predecessor's
    end.  pad = 0 gives the raw runs."""
    if pad < 0:
        raise ValueError(f"pad must be >= 0, got {pad}")
    v = np.asarray(labels.cpu() if torch.is_tensor(labels) else labels).astype(np.int8).ravel()
    d = np.diff(np.concatenate(([0], v, [0])))
    out = []
    for s, c in zip(np.flatnonzero(d == 1).tolist(), np.flatnonzero(d == -1).tolist()):
        lo, hi = max(s - pad, 0), min(c + pad, len(v))
        if out and lo <= out[-1][1]:
            out[-1][1] = hi
        else:
            out.append([lo, hi])
    return [(lo, hi) for lo, hi in out]


def events_to_intervals(events, frame_shift: float):
    """One session's endpointer events in order, [(kind, frame)] with kind 1 = START and 2 = END -> [(start_s, end_s)] with the reference's
    round(k * shift, 2); an interval still open (a START without its END yet) comes last as (start_s, None).  The hysteresis endpointer
    (uvad_endpoint_hyst_step) issues events of the same form: this serves them as they are."""
    ev = np.asarray(events.cpu() if torch.is_tensor(events) else events).reshape(-1, 2).tolist()
    out, lo = [], None
    for kind, frame in ev:
        if kind == 1 and lo is None:
            lo = frame
        elif kind == 2 and lo is not None:
            out.append((round(float(lo * frame_shift), 2), round(float(frame * frame_shift), 2)))
            lo = None
        else:
            raise ValueError(f"events out of order at {(kind, frame)}")
    if lo is not None:
        out.append((round(float(lo * frame_shift), 2), None))
    return out


def split_into_windows(intervals, window: float = 10):
    """predict.py:638-647: cut intervals longer than `window` seconds; drop remainders of 0.1 s or less."""
    out = []
    for s, e in intervals:
        while e - s > window:
            out.append([s, s + window])
            s += window
        if e - s > 0.1:
            out.append([s, e])
    return out


def split_runs(intervals, max_len: int, min_len: int = 0) -> List[Tuple[int, int]]:
    """split_into_windows (predict.py:638-647) on integer FRAMES, in closed form (host; step 3 of uvad_cuts_table, restated): an interval
    [lo, hi) of L frames gives q = (L - 1) // max_len pieces of max_len frames from lo on and a last piece of r = L - q * max_len frames,
    0 < r <= max_len, kept iff r > min_len.  max_len = 0: no splitting (q = 0, r = L).  The reference's window=10 with its 0.1 s rule at
    10 ms frames is max_len=1000, min_len=10."""
    max_len, min_len = int(max_len), int(min_len)
    if max_len < 0 or min_len < 0 or (max_len > 0 and min_len >= max_len):
        raise ValueError(f"need max_len >= 0 and 0 <= min_len (< max_len when splitting), got {max_len}, {min_len}")
    out = []
    for lo, hi in intervals:
        lo, hi = int(lo), int(hi)
        L = hi - lo
        if L < 1:
            continue
        q = (L - 1) // max_len if max_len else 0
        out.extend((lo + j * max_len, lo + (j + 1) * max_len) for j in range(q))
        if L - q * max_len > min_len:
            out.append((lo + q * max_len, hi))
    return out


def cut_table(labels, pad: int, max_len: int = 0, min_len: int = 0) -> List[Tuple[int, int]]:
    """One row of 0/1 labels -> its cuts [(first_frame, end_frame)]: merged_runs, then split_runs.  The host restatement of what
    uvad_cuts_table (VadRuntime.cuts_table) lists for the row, frames only."""
    return split_runs(merged_runs(labels, pad), max_len, min_len)


def cuts_config(buffer: float = 0.0, split: bool = False, window: float = 10.0, min: float = 0.1, frame_shift: float = 0.01,
                hop: int = 160, tail: int = 240, lead: int = 0) -> dict:
    """The reference's get_new_cuts options in seconds -> the integer configuration of uvad_cuts_table: seconds become frames by
    round(x / frame_shift); split=False is max_len = min_len = 0.  hop / tail: samples per frame and the samples a frame sees past its
    hop (160 / 240 for log-mel at 10 ms, 270 / 721 for SincNet)."""
    fr = lambda x: int(round(float(x) / frame_shift))
    return {"pad": fr(buffer), "max_len": fr(window) if split else 0, "min_len": fr(min) if split else 0,
            "hop": int(hop), "lead": int(lead), "tail": int(tail)}


def binarize_config(onset: float = 0.5, offset=None, min_duration_on: float = 0.0, min_duration_off: float = 0.0, pad_onset: float = 0.0,
                    pad_offset: float = 0.0, frame_shift: float = 0.01) -> dict:
    """Hysteresis options in seconds -> the configuration of uvad_binarize (VadRuntime.binarize_open): the two thresholds as they are
    (offset defaults to onset), the durations in frames by int(round(x / frame_shift))."""
    fr = lambda x: int(round(float(x) / frame_shift))
    return {"onset": float(onset), "offset": float(onset if offset is None else offset), "min_on": fr(min_duration_on),
            "min_off": fr(min_duration_off), "pad_on": fr(pad_onset), "pad_off": fr(pad_offset)}


def hysteresis_runs(probs, cfg: dict) -> List[Tuple[int, int]]:
    """One row of probabilities -> its speech intervals [(lo, hi)] in frames under cfg (binarize_config's dict): the host restatement of
    what uvad_binarize (VadRuntime.binarize) lists for the row.  The state turns on at !(p < onset), off at p < offset (compared in f32,
    NaN counts as speech) and holds in between; its runs are widened by pad_on / pad_off and clipped to the row, an interval merges into
    its predecessor when the pause between them is <= 0 or shorter than min_off, and merged intervals shorter than min_on are dropped."""
    onset, offset = np.float32(cfg.get("onset", 0.5)), np.float32(cfg.get("offset", cfg.get("onset", 0.5)))
    min_on, min_off, pad_on, pad_off = (int(cfg.get(k, 0)) for k in ("min_on", "min_off", "pad_on", "pad_off"))
    if not (np.isfinite(onset) and np.isfinite(offset)) or offset > onset or min(min_on, min_off, pad_on, pad_off) < 0:
        raise ValueError(f"need finite offset <= onset and frame counts >= 0, got {cfg}")
    p = np.asarray(probs.cpu() if torch.is_tensor(probs) else probs, np.float32).ravel()
    hi_f, lo_f = ~(p < onset), p < offset
    # the state holds the class of the last frame that was not MID: forward-fill the index of that frame
    idx = np.where(hi_f | lo_f, np.arange(p.size), -1)
    idx = np.maximum.accumulate(idx) if p.size else idx
    v = np.where(idx >= 0, hi_f[np.maximum(idx, 0)], False).astype(np.int8)
    d = np.diff(np.concatenate(([0], v, [0])))
    out = []
    for s, c in zip(np.flatnonzero(d == 1).tolist(), np.flatnonzero(d == -1).tolist()):
        lo, hi = max(s - pad_on, 0), min(c + pad_off, len(v))
        if out and (lo <= out[-1][1] or lo - out[-1][1] < min_off):
            out[-1][1] = max(out[-1][1], hi)
        else:
            out.append([lo, hi])
    return [(lo, hi) for lo, hi in out if hi - lo >= min_on]


def intervals_to_labels(intervals, total_duration: float, frame_shift: float) -> np.ndarray:
    """predict.py:654-663 (get_binary_tensor): ceil(duration/shift) frames, [int(s/shift), int(e/shift)) set to 1."""
    import math
    lab = np.zeros(math.ceil(total_duration / frame_shift), np.uint8)
    for s, e in intervals:
        lab[int(s / frame_shift):int(e / frame_shift)] = 1
    return lab


def detection_error(pred_labels: torch.Tensor, gt_labels: torch.Tensor, runtime=None):
    """(B, T) 0/1 predictions vs ground truth on the GPU -> dict of per-row FA, MD, DER fractions
    (predict.py:666-673 / vad_engine.py:102-105).  The counting runs in uvad_der_counts."""
    if not pred_labels.is_cuda:
        raise RuntimeError("detection_error runs on the GPU only")
    rt = runtime or _shared_runtime(pred_labels.device)
    counts = rt.der_counts(pred_labels, gt_labels).to(torch.float64)
    n = float(pred_labels.shape[1])
    fa, md = counts[:, 0] / n, counts[:, 1] / n
    return {"false_alarm": fa, "missed_detection": md, "detection_error_rate": fa + md}


# ---- scoring against reference labels (uvad_score_*, uvad_intervals_to_labels) ----------------------------------

def supervision_frames(intervals_s, duration: float, frame_shift: float = 0.01, geometry: str = "fbank", num_frames=None) -> np.ndarray:
    """Reference intervals in seconds -> the (n, 2) int32 {start, end} frame table VadRuntime.intervals_to_labels rasterises, with the
    reference's own rounding:
      "fbank"    int(s / shift), int(e / shift) over ceil(duration / shift) frames (get_binary_tensor, predict.py:654-663);
      "sincnet"  supervisions_feature_mask (src/datasets/custom_vad.py:41-75): (round(s * 16000) - SINC_HALF) // 270, with start 0 when
                 s <= 0 and end num_frames when e >= duration (num_frames is required).  SINC_HALF is what the reference's code
                 computes, round(0.5 * 991) = 496; its comment says 495.
    One deviation: a negative index is clamped to 0.  The reference lets numpy wrap it, which silently drops a supervision that starts
    in the first 31 ms.  Ends past the row are cut by the rasteriser (as the reference's slice is)."""
    out = np.zeros((len(intervals_s), 2), np.int32)
    if geometry == "fbank":
        for i, (s, e) in enumerate(intervals_s):
            out[i] = max(int(s / frame_shift), 0), max(int(e / frame_shift), 0)
    elif geometry == "sincnet":
        if num_frames is None:
            raise ValueError("geometry 'sincnet' needs num_frames")
        for i, (s, e) in enumerate(intervals_s):
            st = int((round(s * 16000) - SINC_HALF) // SINC_STEP) if s > 0 else 0
            et = int((round(e * 16000) - SINC_HALF) // SINC_STEP) if e < duration else int(num_frames)
            out[i] = max(st, 0), max(et, 0)
    else:
        raise ValueError(f"unknown geometry {geometry!r} (fbank, sincnet)")
    return out


def _ratio(a, b) -> float:
    return float(a) / float(b) if b else 0.0


def score_metrics(read: dict, prefix: str = "test", point: int = 0) -> dict:
    """VadRuntime.score_read's dict -> what test_step / validation_step log (vad_engine.py:128-202), under the reference's names:
    {prefix}_detection_error_rate, _false_alarm, _missed_detection, _acc, _precision, _recall, _f1_score, _denominator, _loss, at
    operating point `point`.  The values are POOLED over everything accumulated: counts over the scored frames, the loss sum over the
    valid frames.  Lightning instead averages the per-batch values weighted by batch_size=80; for equal-size batches without padding
    the two coincide.  A ratio with a zero denominator is 0 (as torchmetrics); the loss of zero frames is NaN."""
    tp, fp, tn, fn = (int(v) for v in read["counts"][point])
    den = tp + fp + tn + fn
    valid = int(read["valid"])
    return {f"{prefix}_detection_error_rate": _ratio(fp + fn, den),
            f"{prefix}_false_alarm": _ratio(fp, den),
            f"{prefix}_missed_detection": _ratio(fn, den),
            f"{prefix}_acc": _ratio(tp + tn, den),
            f"{prefix}_precision": _ratio(tp, tp + fp),
            f"{prefix}_recall": _ratio(tp, tp + fn),
            f"{prefix}_f1_score": _ratio(2 * tp, 2 * tp + fp + fn),
            f"{prefix}_denominator": float(den),
            f"{prefix}_loss": float(read["loss_sum"]) / valid if valid else float("nan")}


def det_curve(read: dict) -> dict:
    """The threshold sweep of a scoring state: with hist[class][bin] of the raw probabilities, at threshold j / bins (j = 0 .. bins, K = 1)
    the false-alarm frames are the sum of hist[0] over bins >= j and the missed frames the sum of hist[1] over bins < j, exactly, for j < bins; the last entry, j = bins, stands for a threshold above every
    probability (nothing is speech: p = 1 and NaN sit in the last bin).
    -> thresholds (bins + 1,), fa_frames, md_frames (int64), false_alarm_rate = fa / non-speech frames, missed_detection_rate = md / speech
    frames (0 where the class is empty), eer and eer_threshold (where the two rates cross, linearly interpolated), best_threshold and
    best_detection_error_rate (the minimum of (fa + md) / scored frames; the lowest threshold on ties)."""
    hist = np.asarray(read["hist"], np.int64)
    bins = hist.shape[1]
    neg, pos = int(hist[0].sum()), int(hist[1].sum())
    fa = np.concatenate((np.cumsum(hist[0][::-1])[::-1], [0])).astype(np.int64)
    md = np.concatenate(([0], np.cumsum(hist[1]))).astype(np.int64)
    thr = np.arange(bins + 1, dtype=np.float64) / bins
    far = fa / neg if neg else np.zeros(bins + 1)
    mdr = md / pos if pos else np.zeros(bins + 1)
    d = far - mdr                                   # non-increasing in j
    j = int(np.argmax(d <= 0)) if (d <= 0).any() else bins
    if j == 0 or d[j] == 0 or d[j] > 0:
        eer, eer_thr = 0.5 * (far[j] + mdr[j]), thr[j]
    else:
        w = d[j - 1] / (d[j - 1] - d[j])
        eer, eer_thr = far[j - 1] + w * (far[j] - far[j - 1]), thr[j - 1] + w * (thr[j] - thr[j - 1])
    best = int(np.argmin(fa + md))
    return {"thresholds": thr, "fa_frames": fa, "md_frames": md, "false_alarm_rate": far, "missed_detection_rate": mdr,
            "eer": float(eer), "eer_threshold": float(eer_thr), "best_threshold": float(thr[best]),
            "best_detection_error_rate": _ratio(fa[best] + md[best], neg + pos)}


def read_label_file(path: str):
    """A label file in the text form the reference's get_audacity_labels writes (helper.py:135-151), one `start<TAB>end<TAB>LABEL` line
    per speech interval -> [(start_s, end_s)]; blank lines are skipped."""
    out = []
    with open(path) as f:
        for ln, line in enumerate(f, 1):
            parts = line.split()
            if not parts:
                continue
            if len(parts) < 2:
                raise ValueError(f"{path}:{ln}: expected `start<TAB>end<TAB>LABEL`")
            out.append((float(parts[0]), float(parts[1])))
    return out


# ---- the cut-supervision join (uvad_cuts_join): supervisions, transcripts and the reference's report ------------

JOIN_REPORT_NAMES = ("Total Supervisions", "Supervisions in new cuts", "Unique Supervisions in new cuts", "Supervisions not in new cuts",
                     "Supervisions exceeding new cuts", "Supervisions in multiple new cuts", "Empty cuts")


def read_supervisions(path: str):
    """A supervision (or word alignment) file, one `start<TAB>end<TAB>text` line per item -> [(start_s, end_s, text)].  The text is the
    rest of the line, stripped -- it may hold blanks and tabs -- and None when the line has none; blank lines are skipped.  The files
    read_label_file reads are of this form with the label as text."""
    out = []
    with open(path) as f:
        for ln, line in enumerate(f, 1):
            parts = line.strip().split(None, 2)
            if not parts:
                continue
            if len(parts) < 2:
                raise ValueError(f"{path}:{ln}: expected `start<TAB>end<TAB>text`")
            out.append((float(parts[0]), float(parts[1]), parts[2].strip() if len(parts) > 2 else None))
    return out


def cut_transcripts(pairs_per_cut, texts) -> List[str]:
    """The reference's transcript of each cut (predict.py:549-553, the alignment's words at :555-572): the texts of the cut's items in
    the order listed, each followed by one blank, the whole stripped.  pairs_per_cut: for each cut the indices of its items
    (VadRuntime.cuts_join_read); texts: the row's texts by item index.  A text of None is skipped."""
    out = []
    for items in pairs_per_cut:
        text = ""
        for j in items:
            if texts[j] is not None:
                text += texts[j] + " "
        out.append(text.strip())
    return out


def join_report(audit: dict, dataset_name: str, buffer, phase: str) -> str:
    """The text block get_new_cuts prints after a run (predict.py:597-611; its three detection-error lines belong to the scoring stage,
    score_metrics) from an audit of VadRuntime.cuts_join_read -- its "audit" dict (the pooled counters are used) or one row of it."""
    a = audit.get("pooled", audit)
    lines = [f"Dataset: {dataset_name}, Buffer: {buffer}, Phase: {phase}", "", "----------------"]
    lines += [f"{name}: {int(a[name])}" for name in JOIN_REPORT_NAMES]
    return "\n".join(lines) + "\n"


FUSE_MODE_NAMES = ("max", "mean", "vote")


def fuse_config(mode="max", threshold=0.5, decide=None, groups=None, weights=None):
    """A validated configuration of the channel fusion (VadRuntime.fuse_open, predict_vad(fuse=...)): groups is one list of input rows
    per recording (1 .. 255 rows each, every index >= 0); weights None or one list per group of finite values >= 0 that do not sum to
    0; threshold is a member's own speech test and decide the fused value's, both finite.  decide defaults to threshold, or to 0.5
    (a majority) for "vote".  groups may be None where the caller makes them (predict_vad: the channels of each file)."""
    if mode not in FUSE_MODE_NAMES:
        raise ValueError(f"fuse mode must be one of {list(FUSE_MODE_NAMES)}, got {mode!r}")
    if decide is None:
        decide = 0.5 if mode == "vote" else threshold
    for name, v in (("threshold", threshold), ("decide", decide)):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.floating, np.integer)) or not np.isfinite(v):
            raise ValueError(f"fuse {name} must be a finite number, got {v!r}")
    out = {"mode": mode, "threshold": float(threshold), "decide": float(decide), "groups": None, "weights": None}
    if groups is None:
        if weights is not None:
            raise ValueError("fuse weights are given per group: they need groups")
        return out
    gs = [[int(r) for r in g] for g in groups]
    if not gs:
        raise ValueError("fuse needs at least one group")
    for i, g in enumerate(gs):
        if not 1 <= len(g) <= 255:
            raise ValueError(f"a fuse group has 1 .. 255 members, group {i} has {len(g)}")
        if min(g) < 0:
            raise ValueError(f"fuse group {i} names a negative row")
    out["groups"] = gs
    if weights is not None:
        ws = [[float(v) for v in w] for w in weights]
        if len(ws) != len(gs) or any(len(w) != len(g) for w, g in zip(ws, gs)):
            raise ValueError("fuse weights must have the shape of groups")
        for i, w in enumerate(ws):
            if any(not np.isfinite(v) or v < 0 for v in w):
                raise ValueError(f"fuse weights must be finite and >= 0 (group {i})")
            if not sum(w) > 0:
                raise ValueError(f"the fuse weights of group {i} sum to 0")
        out["weights"] = ws
    return out


GROUP_GATE_KEYS = ("decide_frames", "pad", "max_len", "hop", "lead", "tail", "lag_frames", "history", "best_history", "ld_out", "max_seg")


def group_gate_config(group_gate, fuse=None, endpoint=None) -> dict:
    """A validated `group_gate=` of the slot pools (VadRuntime.window_slots_open): a dict with decide_frames (required, 1 .. 2^24: the
    frames of a cut that choose its channel) and any of pad, max_len, hop, lead, tail, lag_frames, history, best_history, ld_out,
    max_seg.  The group gate stands behind the fusion and an endpointer, so it needs fuse= and endpoint=."""
    if not isinstance(group_gate, dict):
        raise ValueError(f"group_gate must be a dict with decide_frames, got {group_gate!r}")
    if fuse is None or endpoint is None:
        raise ValueError("group_gate needs fuse= and endpoint=: it reads the fusion's best bytes and the labels an endpointer finalises")
    extra = set(group_gate) - set(GROUP_GATE_KEYS)
    if extra:
        raise ValueError(f"unknown group_gate parameters {sorted(extra)} {GROUP_GATE_KEYS}")
    D = group_gate.get("decide_frames")
    if isinstance(D, bool) or not isinstance(D, (int, np.integer)) or not 1 <= D <= 1 << 24:
        raise ValueError(f"group_gate needs decide_frames, an integer in [1, 2^24], got {D!r}")
    out = {k: int(v) for k, v in group_gate.items() if v is not None}
    return out
