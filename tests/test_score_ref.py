"""CPU checks of the scoring stage's host side: the numpy restatement (tests/score_ref.py) against brute force -- explicit window sums
for the median, a per-threshold recount for the sweep identity at every j / bins -- supervision_frames against literal transcriptions
of the reference's get_binary_tensor and supervisions_feature_mask, and score_metrics / det_curve on hand-built counts."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import score_ref as sr  # noqa: E402

from uvad_amd import postprocess as pp  # noqa: E402


def _rows(seed, B=4, T=300):
    rng = np.random.default_rng(seed)
    p = rng.random((B, T), dtype=np.float32)
    p[:, ::17] = rng.integers(0, 17, size=p[:, ::17].shape).astype(np.float32) / 16    # exact j / 16, 0 and 1 among them
    runs = np.cumsum(rng.random((B, T)) < 0.05, axis=1) % 2
    return p, runs.astype(np.uint8), [T, 131, 1, 0][:B]


@pytest.mark.parametrize("kernel", [1, 3, 25, 255])
def test_median_labels_against_explicit_window_sums(kernel):
    p, _, _ = _rows(1)
    h = kernel // 2
    for row, n in ((p[0], 300), (p[1], 70), (p[2], 1)):
        x = [not (v < np.float32(0.4)) for v in row[:n]]
        want = [sum(x[max(t - h, 0):min(t + h + 1, n)]) > h for t in range(n)]
        assert sr.median_labels(row[:n], 0.4, kernel).tolist() == want


def test_nan_counts_as_speech_and_lands_in_the_last_bin():
    p = np.array([np.nan, 0.1, 1.0, 0.0, 0.5], np.float32)
    assert sr.median_labels(p, 0.5, 1).tolist() == [True, False, True, False, True]
    assert sr.hist_bins(p, 16).tolist() == [15, 1, 15, 0, 8]
    assert math.isnan(sr.score(p[None], np.ones((1, 5), np.uint8), None, [(0.5, 1)], 0, 2)["loss_sum"])


@pytest.mark.parametrize("collar", [0, 1, 3])
def test_collar_against_the_definition(collar):
    _, g, _ = _rows(2)
    g = g[0] != 0
    n = len(g)
    bounds = [k for k in range(1, n) if g[k - 1] != g[k]]
    want = [not any(k - collar <= t <= k + collar - 1 for k in bounds) for t in range(n)]
    assert sr.scored_mask(g, collar).tolist() == want
    assert sr.scored_mask(g[:1], collar).tolist() == [True]


@pytest.mark.parametrize("bins", [2, 16, 1024])
@pytest.mark.parametrize("collar", [0, 2])
def test_sweep_identity_at_every_threshold(bins, collar):
    """sum of hist[0] over bins >= j == false-alarm frames at threshold j / bins with K = 1, sum of hist[1] over bins < j == missed frames,
    for every j < bins (p = 1 and NaN sit in the last bin and are speech at threshold 1 too: j = bins stands for "above every probability")."""
    p, g, lens = _rows(3)
    r = sr.score(p, g, lens, [(0.5, 1)], collar, bins)
    for j in range(bins):
        at = sr.score(p, g, lens, [(j / bins, 1)], collar, bins)["counts"][0]
        assert r["hist"][0][j:].sum() == at[1] and r["hist"][1][:j].sum() == at[3], j
    d = pp.det_curve(r)
    assert d["fa_frames"][bins // 2] == sr.score(p, g, lens, [(0.5, 1)], collar, bins)["counts"][0][1]
    assert d["fa_frames"][0] == r["hist"][0].sum() and d["md_frames"][bins] == r["hist"][1].sum()


def test_counts_and_loss_against_a_direct_recount():
    p, g, lens = _rows(4)
    r = sr.score(p, g, lens, [(0.5, 25), (0.3, 1)], 0, 16)
    assert r["counts"].sum(axis=1).tolist() == [sum(lens)] * 2 and r["valid"] == sum(lens)
    assert (r["rows"].sum(axis=1) == np.array(lens)).all()
    want = 0.0
    for b, n in enumerate(lens):
        for t in range(n):
            q = float(p[b, t]) if g[b, t] else 1.0 - float(p[b, t])
            want -= max(math.log(q), -100.0) if q > 0 else -100.0
    assert abs(r["loss_sum"] - want) <= 1e-9 * abs(want)
    one = sr.score(np.zeros((1, 5), np.float32), np.ones((1, 5), np.uint8), None, [(0.5, 1)], 0, 2)
    assert one["loss_sum"] == 500.0                                       # p = 0 at g = 1: exactly 100 per frame


def _get_binary_tensor(intervals, total_duration, frame_shift):           # other_vad_metrics.py:299-308, transcribed
    tensor = np.zeros(math.ceil(total_duration / frame_shift))
    for interval in intervals:
        start, end = interval
        start, end = int(start / frame_shift), int(end / frame_shift)
        tensor[start:end] = 1
    return tensor


def _supervisions_feature_mask(sups, duration, num_frames):              # custom_vad.py:41-75, transcribed
    RECEPTIVE_FIELD_1, RECEPTIVE_FIELD_2 = 991, 1261
    STEP = RECEPTIVE_FIELD_2 - RECEPTIVE_FIELD_1
    HALF_DURATION = round(0.5 * RECEPTIVE_FIELD_1)
    mask = np.zeros(num_frames, dtype=np.float32)
    for start, end in sups:
        start_sample = round(start * 16000)
        end_sample = round(end * 16000)
        st = int((start_sample - HALF_DURATION) // STEP) if start > 0 else 0
        et = int((end_sample - HALF_DURATION) // STEP) if end < duration else num_frames
        mask[st:et] = 1.0
    return mask


def _raster(table, n):
    return sr.intervals_to_labels([table], [len(table)], n, None, np.zeros((1, n), np.uint8))[0]


def test_supervision_frames_fbank_matches_get_binary_tensor():
    duration, shift = 7.513, 0.01
    ivs = [(0.0, 0.5), (0.496, 1.2049), (3.3333, 3.3391), (2.0, 1.0), (6.9, 7.513), (7.0, 9.0), (5.005, 5.015)]
    table = pp.supervision_frames(ivs, duration, frame_shift=shift)
    assert table.dtype == np.int32 and table.shape == (len(ivs), 2)
    want = _get_binary_tensor(ivs, duration, shift)
    assert (_raster(table, len(want)) == want).all()
    assert (_raster(pp.supervision_frames(ivs, duration, frame_shift=0.02), math.ceil(duration / 0.02)) == _get_binary_tensor(ivs, duration, 0.02)).all()


def test_supervision_frames_sincnet_matches_supervisions_feature_mask():
    duration, nf = 5.0, 293
    ivs = [(0.0, 0.7), (0.65, 1.3), (2.0, 2.0169), (2.5, 2.5168), (4.2, 5.0), (3.0, 5.5), (0.05, 0.4)]     # touch 0 and duration, overlap, between frames
    table = pp.supervision_frames(ivs, duration, geometry="sincnet", num_frames=nf)
    assert (_raster(table, nf) == _supervisions_feature_mask(ivs, duration, nf)).all()
    # the stated deviation: a supervision that starts inside the first 31 ms has a negative index in the reference (numpy wraps it and the
    # supervision is dropped); here it is clamped to 0 and kept
    early = [(0.02, 1.0)]
    t = pp.supervision_frames(early, duration, geometry="sincnet", num_frames=nf)
    assert t[0, 0] == 0 and _raster(t, nf)[:3].tolist() == [1, 1, 1]
    assert _supervisions_feature_mask(early, duration, nf).sum() < _raster(t, nf).sum()
    with pytest.raises(ValueError):
        pp.supervision_frames(ivs, duration, geometry="sincnet")
    with pytest.raises(ValueError):
        pp.supervision_frames(ivs, duration, geometry="mel")


def _read(counts, hist, loss=0.0, valid=None):
    counts = np.array([counts], np.int64)
    return {"counts": counts, "hist": np.array(hist, np.int64), "loss_sum": loss, "valid": int(counts.sum()) if valid is None else valid}


def test_metrics_of_a_perfect_detector():
    r = _read([40, 0, 60, 0], [[60, 0, 0, 0], [0, 0, 0, 40]], loss=1.5)
    m = pp.score_metrics(r, prefix="test")
    assert set(m) == {"test_" + k for k in ("detection_error_rate", "false_alarm", "missed_detection", "acc", "precision", "recall", "f1_score",
                                            "denominator", "loss")}
    assert (m["test_detection_error_rate"], m["test_false_alarm"], m["test_missed_detection"]) == (0.0, 0.0, 0.0)
    assert (m["test_acc"], m["test_precision"], m["test_recall"], m["test_f1_score"]) == (1.0, 1.0, 1.0, 1.0)
    assert m["test_denominator"] == 100.0 and m["test_loss"] == 0.015
    d = pp.det_curve(r)
    assert d["eer"] == 0.0 and d["best_detection_error_rate"] == 0.0 and 0.25 <= d["best_threshold"] <= 0.75
    assert d["thresholds"].tolist() == [0.0, 0.25, 0.5, 0.75, 1.0]
    assert d["false_alarm_rate"].tolist() == [1.0, 0.0, 0.0, 0.0, 0.0] and d["missed_detection_rate"].tolist() == [0.0, 0.0, 0.0, 0.0, 1.0]


def test_metrics_of_an_all_speech_detector():
    r = _read([30, 70, 0, 0], [[0, 0, 0, 70], [0, 0, 0, 30]])
    m = pp.score_metrics(r, prefix="val")
    assert m["val_false_alarm"] == 0.7 and m["val_missed_detection"] == 0.0 and m["val_detection_error_rate"] == 0.7
    assert m["val_recall"] == 1.0 and m["val_precision"] == 0.3 and m["val_acc"] == 0.3 and abs(m["val_f1_score"] - 60 / 130) < 1e-15
    d = pp.det_curve(r)
    assert d["fa_frames"].tolist() == [70, 70, 70, 70, 0] and d["md_frames"].tolist() == [0, 0, 0, 0, 30]
    assert d["best_threshold"] == 1.0 and d["best_detection_error_rate"] == 0.3          # calling nothing speech beats calling everything speech
    assert 0.0 <= d["eer"] <= 1.0 and 0.75 <= d["eer_threshold"] <= 1.0


def test_metrics_with_an_empty_reference_and_zero_denominators():
    r = _read([0, 0, 50, 0], [[50, 0], [0, 0]])
    m = pp.score_metrics(r)
    assert m["test_precision"] == 0.0 and m["test_recall"] == 0.0 and m["test_f1_score"] == 0.0 and m["test_acc"] == 1.0
    d = pp.det_curve(r)
    assert d["missed_detection_rate"].tolist() == [0.0, 0.0, 0.0] and d["false_alarm_rate"].tolist() == [1.0, 0.0, 0.0]
    nothing = pp.score_metrics(_read([0, 0, 0, 0], [[0, 0], [0, 0]]))
    assert nothing["test_detection_error_rate"] == 0.0 and nothing["test_denominator"] == 0.0 and math.isnan(nothing["test_loss"])
    assert pp.det_curve(_read([0, 0, 0, 0], [[0, 0], [0, 0]]))["eer"] == 0.0


def test_label_file_round_trip(tmp_path):
    f = tmp_path / "rec.txt"
    f.write_text("0.0\t1.25\tSPC\n\n3.5\t4.0\tSPC\n")
    assert pp.read_label_file(str(f)) == [(0.0, 1.25), (3.5, 4.0)]
