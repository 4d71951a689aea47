"""``predict_vad(**config)``: the reference's predict entry point (src/scripts/predict.py:22-110)
with its lhotse / Lightning plumbing replaced by a manifest-free source.  Flow kept from the
reference: seed -> model (checkpoint or seeded weights) -> batches bounded by ``max_duration``
seconds -> ``VadModel.predict_step`` semantics (probabilities -> threshold 0.5 -> median filter ->
0/1 labels) -> per-recording speech intervals (predict.py:472-490).

Cut geometry (``window_seconds``, default = the reference's 5.0):
  the reference never shows the model a whole recording.  Every recording is cut into 5 s windows,
  a tail of <= 3 s is dropped (``cut_into_windows(duration=5).filter(lambda cut: cut.duration > 3)``,
  src/datasets/ami/utils.py:107), features are computed per window and padded to 5 s
  (``.pad(duration=5.0)``, ami/utils.py:163: lhotse pads log-mel features with log(1e-10)), the BiLSTM
  starts from zero state in every window, the median filter runs per window row
  (vad_engine.py:204-211) and the rows are laid end to end and cut to ceil(duration / frame_shift) + 1
  frames per recording (predict.py:451-458).  ``window_seconds=5.0`` reproduces exactly that, so
  a trained checkpoint gives the reference's labels; ``window_seconds=None`` runs the model over whole
  recordings instead (one BiLSTM pass per recording: different numbers for anything longer than a
  window -- an explicit option, not the default).

Every batch goes through the fused hot path: PCM (int16 straight from the wav file, or f32) ->
``uvad_forward[_i16]`` (features stay in the workspace; SincNet: ``uvad_forward_wav[_i16]``) -> ``uvad_median_filter`` ->
``uvad_label_runs``; several batches are kept in flight with ``ForwardPipeline`` when there is more than one.

``binarize={...}`` (seconds; ``BINARIZE_DEFAULTS``) replaces the last two steps by ``uvad_binarize``: hysteresis between an onset and an
offset threshold, padding, pauses shorter than ``min_duration_off`` filled and intervals shorter than ``min_duration_on`` dropped.  The
default, ``None``, leaves every path as described above."""
import json
import math
import os
import struct
import wave
from typing import List

import numpy as np
import torch

from .engine import VadModel
from .features import FbankConfig
from .pipeline import ForwardPipeline
from .postprocess import (binarize_config, cuts_config, labels_to_intervals_batch, median_filter, sincnet_frame_times,
                          sincnet_labels_to_intervals, sliding_weights)
from .sincnet import SincNet
from .synth import seed_weights, synth_pcm

LOG_EPS_PAD = math.log(1e-10)   # lhotse's padding value for log-mel features (LOG_EPSILON)


def read_wav_int16(path: str, sample_rate: int = 16000) -> np.ndarray:
    with wave.open(path, "rb") as w:
        if w.getframerate() != sample_rate or w.getsampwidth() != 2:
            raise ValueError(f"{path}: need {sample_rate} Hz 16-bit PCM")
        pcm = np.frombuffer(w.readframes(w.getnframes()), dtype="<i2")
        if w.getnchannels() > 1:
            pcm = pcm.reshape(-1, w.getnchannels())[:, 0]
    return np.ascontiguousarray(pcm)


def read_audio(path: str):
    """A small RIFF/WAVE reader for what telephone audio comes as: format tags 1 (16-bit linear PCM), 6 (G.711 A-law) and 7 (G.711
    mu-law), any channel count and sample rate (Python's ``wave`` refuses tags 6 and 7).  -> (raw, (encoding, channels, rate)): raw is
    the interleaved samples as stored, shape (frames, channels), int16 for "int16" and uint8 for "alaw" / "ulaw" -- undecoded: the
    ingest stage (VadRuntime.ingest) decodes, de-interleaves and resamples on the GPU."""
    with open(path, "rb") as f:
        blob = f.read()
    if len(blob) < 12 or blob[:4] != b"RIFF" or blob[8:12] != b"WAVE":
        raise ValueError(f"{path}: not a RIFF/WAVE file")
    fmt = data = None
    pos = 12
    while pos + 8 <= len(blob):
        cid, size = blob[pos:pos + 4], struct.unpack("<I", blob[pos + 4:pos + 8])[0]
        body = blob[pos + 8:pos + 8 + size]
        if cid == b"fmt ":
            fmt = body
        elif cid == b"data":
            data = body
            break
        pos += 8 + size + (size & 1)      # chunks are word aligned
    if fmt is None or data is None or len(fmt) < 16:
        raise ValueError(f"{path}: no fmt / data chunk")
    tag, channels, rate, _, _, bits = struct.unpack("<HHIIHH", fmt[:16])
    if tag == 0xFFFE and len(fmt) >= 26:  # WAVE_FORMAT_EXTENSIBLE: the tag is the head of the sub-format GUID
        tag = struct.unpack("<H", fmt[24:26])[0]
    if channels < 1 or rate < 1:
        raise ValueError(f"{path}: bad channel count / sample rate")
    if tag == 1 and bits == 16:
        encoding, dtype = "int16", "<i2"
    elif tag in (6, 7) and bits == 8:
        encoding, dtype = ("alaw" if tag == 6 else "ulaw"), np.uint8
    else:
        raise ValueError(f"{path}: format tag {tag} with {bits} bits per sample is not supported (16-bit PCM, A-law, mu-law)")
    width = channels * np.dtype(dtype).itemsize
    raw = np.frombuffer(data[:len(data) // width * width], dtype=dtype).reshape(-1, channels)
    return raw.copy(), (encoding, channels, rate)


def _wav_recordings(path: str, channels: str, rt, sample_rate: int = 16000):
    """The recordings of one wav file.  A file read_wav_int16 accepts (16 kHz, 16-bit) whose first channel is all that is asked for
    takes that path: int16 samples, converted on the GPU by the _i16 entry points.  Anything else -- another rate, G.711, every
    channel of a multi-channel file -- goes through read_audio and the ingest stage to f32 rows at 16 kHz."""
    rid = os.path.basename(path)
    try:
        with wave.open(path, "rb") as w:
            plain = w.getframerate() == sample_rate and w.getsampwidth() == 2 and (channels == "first" or w.getnchannels() == 1)
    except (wave.Error, EOFError):
        plain = False
    if plain:
        return [{"id": rid + ("-ch0" if channels == "all" else ""), "pcm": read_wav_int16(path, sample_rate), "file": rid, "channel": 0}]
    raw, (encoding, nch, rate) = read_audio(path)
    ig = getattr(rt, "_ingest", None) or {}
    if (ig.get("encoding"), ig.get("channels"), ig.get("sample_rate")) != (encoding, nch, rate):   # files of one kind configure once
        rt.ingest_configure(encoding, nch, rate)
    # (channels, samples at 16 kHz) f32, back on the host: the recordings are cut into windows and batched there, like the int16 ones,
    # and each batch is uploaded again -- one extra round trip per file, kept so that both kinds of recording share one batching path
    rows = rt.ingest(torch.from_numpy(raw[None]).to(rt.device)).cpu().numpy()
    if channels == "first":
        return [{"id": rid, "pcm": rows[0], "file": rid, "channel": 0}]
    return [{"id": f"{rid}-ch{c}", "pcm": rows[c], "file": rid, "channel": c} for c in range(nch)]


def _resolve_device(name: str) -> torch.device:
    if name in ("gpu", "cuda"):
        if not torch.cuda.is_available():
            raise RuntimeError("config.device='gpu' but no HIP device is visible; this package has no CPU path")
        return torch.device("cuda", torch.cuda.current_device())
    raise RuntimeError(f"config.device={name!r}: the VAD path runs in HIP kernels only (use 'gpu'); "
                       "the CPU restatement lives in oracle/ and is test infrastructure")


def cut_into_windows(num_samples: int, window: int, min_keep: int):
    """[(start, length)] of the reference's cuts of one recording: consecutive `window`-sample pieces, the last one
    shorter; pieces of <= min_keep samples are dropped (ami/utils.py:107)."""
    out = []
    for start in range(0, num_samples, window):
        n = min(window, num_samples - start)
        if n > min_keep:
            out.append((start, n))
    return out


def pack_ragged_batches(lengths, max_samples: int):
    """Ragged batches of whole recordings (predict_vad with ragged_batches): indices sorted by length (longest first, ties by index),
    cut into consecutive groups whose PADDED size -- rows x the group's longest row -- stays within max_samples (a recording longer
    than that runs alone).  Each group is one uvad_forward_lens call; a row's results are those of the recording alone."""
    order = sorted(range(len(lengths)), key=lambda i: (-lengths[i], i))
    batches, cur = [], []
    for i in order:
        if cur and (len(cur) + 1) * lengths[cur[0]] > max_samples:   # cur[0] is the group's longest row
            batches.append(cur)
            cur = []
        cur.append(i)
    if cur:
        batches.append(cur)
    return batches


def open_pipeline(net, device, depth: int):
    """ForwardPipeline with as many steps in flight as the device proves concurrent: the constructor raises when it cannot find
    `depth` pairwise-concurrent HIP streams (GPU_MAX_HW_QUEUES of 1 or 2, a shared or restricted device); fewer steps in flight
    give the same numbers, so the depth is halved down to 1 and below that the caller runs batch after batch (returns None)."""
    while depth > 1:
        try:
            return ForwardPipeline(net, device, depth=depth)
        except RuntimeError as e:
            if "concurrent HIP streams" not in str(e):
                raise
            print(f"predict_vad: {e}; continuing with {depth // 2} batch(es) in flight")
            depth //= 2
    return None


def _write_results(results, kwargs):
    results.sort(key=lambda r: r["recording_id"])

    out_dir = kwargs.get("predict_output_dir") or ""
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, "predictions.json"), "w") as f:
            json.dump([{"recording_id": r["recording_id"], "num_frames": r["num_frames"],
                        "speech_frames": int(r["labels"].sum()), "intervals": r["intervals"],
                        **({k: r[k] for k in ("cuts", "audit", "audit_words") if k in r})} for r in results], f, indent=1)
    for r in results:
        print(f"{r['recording_id']}: {r['num_frames']} frames, {int(r['labels'].sum())} speech, {len(r['intervals'])} intervals")
    return results


CUTS_DEFAULTS = {"buffer": 0.0, "split": False, "window": 10.0, "min": 0.1, "write_dir": None}


def _write_wav_int16(path: str, x: np.ndarray, sample_rate: int = 16000):
    if x.dtype != np.int16:   # f32 in [-1, 1): the value an int16 file would have held
        x = np.clip(np.rint(x.astype(np.float64) * 32768.0), -32768, 32767).astype(np.int16)
    with wave.open(path, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(sample_rate)
        w.writeframes(x.astype("<i2").tobytes())


def _join_items(source, rec_ids, nsamp, frames, sincnet, shift, sr):
    """predict_vad(supervisions= / alignments=): {recording_id: path or [(start_s, end_s, text)]} for a group's recordings -> (intervals
    (B, max_iv, 2) int32 frames, counts (B,), texts per row): seconds become frames through supervision_frames with the geometry of the
    model in use; a recording without an entry has no items."""
    from .postprocess import read_supervisions, supervision_frames
    rows = []
    for rid in rec_ids:
        items = source.get(rid, [])
        rows.append(read_supervisions(items) if isinstance(items, (str, os.PathLike)) else [tuple(it) for it in items])
    max_iv = max((len(r) for r in rows), default=0)
    iv = np.zeros((len(rows), max_iv, 2), np.int32)
    for b, r in enumerate(rows):
        if r:
            iv[b, :len(r)] = supervision_frames([(it[0], it[1]) for it in r], nsamp[b] / float(sr), frame_shift=shift,
                                                geometry="sincnet" if sincnet else "fbank", num_frames=frames[b])
    return iv, np.asarray([len(r) for r in rows], np.int32), [[it[2] if len(it) > 2 else None for it in r] for r in rows]


def _attach_cuts(results, recs, dev_labels, rt, cuts, sincnet, frame_shift, device, max_samples, sr=16000, supervisions=None, alignments=None,
                 dev_best=None):
    """predict_vad(cuts=...): the tail of the reference's get_new_cuts on the device.  results[i], recs[i] and dev_labels[i] (the
    recording's whole-row labels, a 1-D tensor on the GPU, or None when it has no frame) belong together.  Recordings are grouped within
    the max_duration budget; a group is one uvad_cuts_table call on its padded label rows, and its table is the only thing that crosses
    to the host -- with write_dir also one uvad_cuts_gather of the group's audio, written as one 16 kHz wav per cut.  Every result gains
    "cuts": [(start_s, end_s, first_sample, n_samples)].
    With supervisions and / or alignments ({recording_id: path or [(start_s, end_s, text)]}) each group also runs uvad_cuts_join on its
    table, on the device -- supervisions by overlap, an alignment's words by containment -- and every cut becomes a dict {"start", "end",
    "first_sample", "n_samples", "supervisions": indices into the recording's list, "text"} (with alignments also "words", whose text
    replaces the supervisions' for a recording that has an alignment), every result gains "audit": the reference's seven counters for that recording (postprocess.join_report prints them).
    With dev_best (predict_vad(fuse=...): per result the best-channel row uvad_fuse wrote, on the GPU; recs[i]["channels"] the audio of
    every channel) one uvad_fuse_pick on each group's table names the channel of each cut, the audio written is gathered from that
    channel's row, and every cut is a dict with "channel"."""
    from .postprocess import cut_transcripts
    join = supervisions is not None or alignments is not None
    fused = dev_best is not None
    unknown = set(cuts) - set(CUTS_DEFAULTS)
    if unknown:
        raise ValueError(f"unknown cuts option(s) {sorted(unknown)} (known: {sorted(CUTS_DEFAULTS)})")
    opt = {**CUTS_DEFAULTS, **cuts}
    hop = 270 if sincnet else int(round(frame_shift * sr))
    tail = 721 if sincnet else max(400 - hop, 0)          # what a frame sees past its hop: 991 - 270, frame_len - hop
    shift = hop / float(sr) if sincnet else frame_shift
    cfg = cuts_config(opt["buffer"], opt["split"], opt["window"], opt["min"], frame_shift=shift, hop=hop, tail=tail)
    if opt["write_dir"]:
        os.makedirs(opt["write_dir"], exist_ok=True)
    for r in results:
        r["cuts"] = []
    have = [i for i in range(len(results)) if dev_labels[i] is not None and dev_labels[i].numel()]
    lengths = [len(recs[i]["pcm"]) for i in have]
    for group in pack_ragged_batches(lengths, max_samples):
        idx = [have[g] for g in group]
        T = max(int(dev_labels[i].numel()) for i in idx)
        lab = torch.zeros((len(idx), T), dtype=torch.uint8, device=device)
        for r, i in enumerate(idx):
            lab[r, :dev_labels[i].numel()] = dev_labels[i].to(torch.uint8)
        frames = [int(dev_labels[i].numel()) for i in idx]
        nsamp = [len(recs[i]["pcm"]) for i in idx]
        S = max(nsamp)
        ct = rt.cuts_open(**cfg)
        rt.cuts_table(lab, lengths=frames, nsamp=nsamp, S=S, cuts=ct)
        tab = rt.cuts_read(ct)
        picks = ptab = None
        if fused:   # the channel of each cut: one more launch on the table where it lies; the group's channels are rows base .. base + C
            base = np.concatenate([[0], np.cumsum([len(recs[i]["channels"]) for i in idx])]).astype(int)
            best = torch.zeros((len(idx), T), dtype=torch.uint8, device=device)
            for r, i in enumerate(idx):
                best[r, :dev_best[i].numel()] = dev_best[i]
            fz = rt.fuse_open([list(range(base[r], base[r + 1])) for r in range(len(idx))])
            ptab, pk = rt.fuse_pick(best, ct, state=fz)
            picks = pk[:len(tab)].cpu().numpy()
        joined = {}
        for name, source, mode in (("supervisions", supervisions, "overlap"), ("words", alignments, "inside")):
            if source is not None:   # one more launch on the table where it lies; the pair lists and eight counters a row cross to the host
                iv, counts, texts = _join_items(source, [recs[i]["id"] for i in idx], nsamp, frames, sincnet, shift, sr)
                rt.cuts_join(ct, iv, counts, mode=mode, rows=len(tab))
                joined[name] = (rt.cuts_join_read(ct), texts, [recs[i]["id"] in source for i in idx])
        batch = lens = None
        if opt["write_dir"] and len(tab):
            audio = [(r, pcm) for r, i in enumerate(idx) for pcm in (recs[i]["channels"] if fused else [recs[i]["pcm"]])]   # (row of idx, samples)
            mixed = len({pcm.dtype for _, pcm in audio}) > 1
            i16 = not mixed and audio[0][1].dtype == np.int16
            x = torch.zeros((len(audio), S), dtype=torch.int16 if i16 else torch.float32, device=device)
            for k, (r, pcm) in enumerate(audio):
                row = torch.from_numpy(np.array(pcm)).to(device)
                x[k, :nsamp[r]] = row.float() / 32768.0 if mixed and row.dtype == torch.int16 else row
            batch, lens = rt.cuts_gather(x, ct, "samples", ld_out=-(-max(int(tab["n_samples"].max()), 1) // 8) * 8, rows=len(tab), table=ptab)
            batch, lens = batch.cpu().numpy(), lens.cpu().numpy()
        for k, c in enumerate(tab):
            res = results[idx[int(c["row"])]]
            f, nf = int(c["first_frame"]), int(c["n_frames"])
            entry = (round(f * shift, 6), round((f + nf) * shift, 6), int(c["first_sample"]), int(c["n_samples"]))
            if join or fused:
                entry = dict(zip(("start", "end", "first_sample", "n_samples"), entry))
            if fused:
                entry["channel"] = int(picks[k])
            if join:
                for name, (read, texts, listed) in joined.items():
                    entry[name] = read["pairs_per_cut"][k]
                    if "text" not in entry or listed[int(c["row"])]:   # the words supply the text of a recording that has an alignment
                        entry["text"] = cut_transcripts([entry[name]], texts[int(c["row"])])[0]
            res["cuts"].append(entry)
            if batch is not None:
                _write_wav_int16(os.path.join(opt["write_dir"], f"{res['recording_id']}_{int(c['index']):04d}.wav"), batch[k, :lens[k]], sr)
        for name, (read, _, _) in joined.items():
            for r, i in enumerate(idx):
                results[i]["audit" if name == "supervisions" or supervisions is None else "audit_words"] = read["audit"]["rows"][r]
    for source, key in ((supervisions, "audit"), (alignments, "audit" if supervisions is None else "audit_words")):
        if source is not None:
            for i, res in enumerate(results):   # a recording without a frame has no cut: all of its items are "not in new cuts"
                if key not in res:
                    n = int(_join_items(source, [recs[i]["id"]], [0], [0], False, shift, sr)[1][0])
                    res[key] = {name: (n if k in (0, 4) else 0) for name, k in rt.JOIN_AUDIT_NAMES}


BINARIZE_DEFAULTS = {"onset": 0.5, "offset": None, "min_duration_on": 0.0, "min_duration_off": 0.0, "pad_onset": 0.0, "pad_offset": 0.0}


def _binarize_frames(binarize, sincnet, frame_shift, sr=16000):
    """predict_vad(binarize=...): the options in seconds -> uvad_binarize's configuration in frames (10 ms log-mel frames; the SincNet
    model's 270-sample hop)."""
    unknown = set(binarize) - set(BINARIZE_DEFAULTS)
    if unknown:
        raise ValueError(f"unknown binarize option(s) {sorted(unknown)} (known: {sorted(BINARIZE_DEFAULTS)})")
    return binarize_config(**{**BINARIZE_DEFAULTS, **binarize}, frame_shift=270.0 / sr if sincnet else frame_shift)


def _binarize_post(rt, cfg, probs, frames, durations, sincnet, frame_shift):
    """The decision stage of predict_vad(binarize=...) for one batch: probs (B, T) on the GPU with `frames` valid frames per row ->
    (labels (B, T) uint8 on the GPU, per-row [(start_s, end_s)]).  One uvad_binarize call; its interval table is the only thing that
    crosses to the host, where an interval [lo, hi) is given in seconds as the median path gives the run [lo, hi): round(lo * shift, 2)
    and round((hi - 1) * shift, 2) for log-mel frames, sincnet_frame_times(lo, hi - 1) for the waveform model, kept iff end - start > 0."""
    st = rt.binarize_open(**cfg)
    lab, _, _ = rt.binarize(probs, lengths=frames, state=st)
    out = []
    for r, row in enumerate(rt.binarize_read(st)):
        ivs = []
        for lo, hi in row:
            if sincnet:
                s, e = sincnet_frame_times(lo, hi - 1, durations[r])
            else:
                s, e = round(float(lo * frame_shift), 2), round(float((hi - 1) * frame_shift), 2)
            if e - s > 0.0:
                ivs.append((s, e))
        out.append(ivs)
    return lab, out


def sliding_geometry(rt, sincnet: bool, window_seconds: float, hop_seconds: float, frame_shift: float, sr: int = 16000):
    """(W, Hf) in frames of predict_vad's sliding path: the frames of one window of window_seconds -- 500 log-mel frames, 293 of the
    waveform model for the reference's 5 s -- and the hop rounded to whole frames (10 ms log-mel frames; 270-sample SincNet frames)."""
    wn = int(round(window_seconds * sr))
    W = rt.sincnet_num_frames(wn) if sincnet else rt.num_frames(wn)
    Hf = int(round(hop_seconds * sr / 270.0)) if sincnet else int(round(hop_seconds / frame_shift))
    if W < 1 or not 1 <= Hf <= W:
        raise ValueError(f"hop_seconds={hop_seconds} gives a hop of {Hf} frames: need 1 <= hop <= window = {W} frames")
    return W, Hf


def _predict_sliding(recs, rt, sincnet, kwargs, window_s, hop_s, frame_shift, med_window, device, sr=16000, dev_labels=None, binarize=None,
                     dev_probs=None):
    """predict_vad with hop_seconds: whole recordings as ragged [R][S_max] batches within the max_duration budget, overlapping windows
    aggregated on the device (uvad_sliding_forward[_wav][_i16]), then the lens median filter and run-length kernels on the frame counts
    the call returned.  Every recording is copied into its row of the device batch by itself: nothing is stacked on the host."""
    W, Hf = sliding_geometry(rt, sincnet, window_s, hop_s, frame_shift, sr)
    rt.sliding_configure(W, Hf, sliding_weights(kwargs.get("sliding_weights", "hamming"), W))
    group = int(kwargs.get("sliding_group", 512))
    results = [None] * len(recs)
    lengths = [len(r["pcm"]) for r in recs]
    min_samples = 991 if sincnet else 1
    for batch in pack_ragged_batches(lengths, int(kwargs["max_duration"] * sr)):
        smax = max(lengths[i] for i in batch)
        if smax < min_samples:   # nothing in this batch holds a frame
            for i in batch:
                results[i] = {"recording_id": recs[i]["id"], "num_frames": 0, "labels": np.zeros(0, np.uint8), "probs": np.zeros(0, np.float32),
                              "intervals": []}
            continue
        mixed = len({recs[i]["pcm"].dtype for i in batch}) > 1   # int16 rows beside ingested f32 ones: read as q / 32768
        i16 = not mixed and recs[batch[0]]["pcm"].dtype == np.int16
        x = torch.zeros((len(batch), smax), dtype=torch.int16 if i16 else torch.float32, device=device)
        for r, i in enumerate(batch):
            row = torch.from_numpy(np.array(recs[i]["pcm"])).to(device)
            x[r, :lengths[i]] = row.float() / 32768.0 if mixed and row.dtype == torch.int16 else row
        nsamp = [lengths[i] for i in batch]
        probs, frames = (rt.sliding_forward_wav if sincnet else rt.sliding_forward)(x, nsamp, group=group)
        fr = frames.tolist()
        if binarize is not None:   # uvad_binarize in place of the median filter and the run walk
            lab, ivs = _binarize_post(rt, binarize, probs, frames, [n / sr for n in nsamp], sincnet, frame_shift)
        else:
            lab = median_filter(probs, window=med_window, runtime=rt, lengths=frames)         # uvad_median_filter_lens
            if sincnet:
                ivs = [sincnet_labels_to_intervals(lab[r, :fr[r]], nsamp[r] / sr, runtime=rt) if fr[r] else [] for r in range(len(batch))]
            else:
                ivs = labels_to_intervals_batch(lab, frame_shift, runtime=rt, lengths=frames)     # uvad_label_runs_lens
        for r, i in enumerate(batch):
            results[i] = {"recording_id": recs[i]["id"], "num_frames": int(fr[r]), "labels": lab[r, :fr[r]].cpu().numpy().astype(np.uint8),
                          "probs": probs[r, :fr[r]].cpu().numpy(), "intervals": ivs[r]}
            if dev_labels is not None:
                dev_labels[i] = lab[r, :fr[r]]
            if dev_probs is not None:
                dev_probs[i] = probs[r, :fr[r]]
    return results


def _fuse_recordings(results, recs, dev_probs, rt, fuse, binarize, sincnet, frame_shift, med_window, device, sr=16000):
    """predict_vad(fuse=...): the channel rows of each file put back together on the device.  results[i], recs[i] and dev_probs[i] (the
    channel's probabilities, a 1-D tensor on the GPU, or None when it has no frame) belong together; recs carry "file" and "channel".
    One uvad_fuse over all channel rows, one group per file; then the decision on the fused rows as the ragged route decides a whole
    row: uvad_binarize with binarize=, else the lens median filter and the run walk.  -> (results, recs, dev_labels, dev_best), one
    entry per file: the result has the id without -chK, "probs" the fused row, "channels" and "channel_stats" (per channel {valid,
    speech, agree, best} frames); recs[i]["channels"] holds every channel's audio for the cuts."""
    files = []
    for i, r in enumerate(recs):
        if not files or files[-1][0] != r["file"]:
            files.append((r["file"], []))
        files[-1][1].append(i)
    frames = [0 if p is None else int(p.numel()) for p in dev_probs]
    T = max(max(frames), 1)
    x = torch.zeros((len(recs), T), dtype=torch.float32, device=device)
    for i, p in enumerate(dev_probs):
        if frames[i]:
            x[i, :frames[i]] = p
    st = rt.fuse_open([idx for _, idx in files], **{k: v for k, v in fuse.items() if k in ("mode", "threshold", "decide")})
    fused, glens, _, best, _ = rt.fuse(x, lengths=frames, state=st, labels=False)
    gl = glens.cpu().tolist()
    stats = rt.fuse_read(st)
    nsamp = [max(len(recs[i]["pcm"]) for i in idx) for _, idx in files]
    if binarize is not None:
        lab, ivs = _binarize_post(rt, binarize, fused, gl, [n / sr for n in nsamp], sincnet, frame_shift)
    else:
        lab = median_filter(fused, window=med_window, runtime=rt, lengths=gl)
        if sincnet:
            ivs = [sincnet_labels_to_intervals(lab[g, :gl[g]], nsamp[g] / sr, runtime=rt) if gl[g] else [] for g in range(len(files))]
        else:
            ivs = labels_to_intervals_batch(lab, frame_shift, runtime=rt, lengths=gl)
    out, new_recs, dev_labels, dev_best = [], [], [], []
    for g, (name, idx) in enumerate(files):
        L = gl[g]
        out.append({"recording_id": name, "num_frames": L, "labels": lab[g, :L].cpu().numpy().astype(np.uint8), "probs": fused[g, :L].cpu().numpy(),
                    "intervals": ivs[g], "channels": len(idx),
                    "channel_stats": [dict(stats[g][k], channel=recs[i]["channel"]) for k, i in enumerate(idx)]})
        new_recs.append({"id": name, "pcm": recs[idx[0]]["pcm"], "channels": [recs[i]["pcm"] for i in idx]})
        dev_labels.append(lab[g, :L] if L else None)
        dev_best.append(best[g, :L])
    return out, new_recs, dev_labels, dev_best


def predict_vad(**kwargs):
    assert kwargs["model_name"] in kwargs["supported_models"], \
        f"Invalid model {kwargs['model_name']}. Model should be one of {kwargs['supported_models']}"
    if kwargs["feature_extractor"] not in ("fbank", "sincnet"):
        raise NotImplementedError("feature_extractor must be 'fbank' (log-mel + PyanNet2) or 'sincnet' (waveform PyanNet); "
                                  "the wav2vec2 / hubert encoders are outside the accelerated path")
    sincnet = kwargs["feature_extractor"] == "sincnet"   # the reference's custom_vad path: the model consumes raw audio
    torch.manual_seed(kwargs["seed"])
    np.random.seed(kwargs["seed"])
    device = _resolve_device(kwargs["device"])
    frame_shift = kwargs["frame_shift"]
    model_dict = dict(kwargs["model_dict"])
    sr = 16000

    if kwargs["load_checkpoint"]:
        model = VadModel.load_from_checkpoint(checkpoint_path=kwargs["checkpoint_path"],
                                              model_name=kwargs["model_name"], model_dict=model_dict)
    else:
        model = VadModel(model_name=kwargs["model_name"], model_dict=model_dict)
        seed_weights(model.model, kwargs.get("weights_seed", 1234), kwargs.get("weights_scale", 4.0))
    model = model.to(device).eval()
    net = model.model
    if not sincnet:
        net.attach_fbank(FbankConfig(sampling_rate=sr, num_filters=net.encoding_dim, window_type=kwargs.get("window_type", "povey"),
                                     frame_shift=frame_shift, device="cuda"))

    src = kwargs["input"]
    recs: List[dict] = []
    if src["kind"] == "wav":
        channels = src.get("channels", "first")
        if channels not in ("first", "all"):
            raise ValueError(f"input channels must be 'first' or 'all', got {channels!r}")
        for p in src["paths"]:
            recs.extend(_wav_recordings(p, channels, net.runtime(device), sr))             # int16: converted on the GPU
    elif src["kind"] == "synthetic":
        S = int(round(src["seconds"] * sr))
        pcm = synth_pcm(src["num_utterances"], S, seed=src["seed"])
        recs = [{"id": f"synthetic-{src['seed'] + i}", "pcm": pcm[i]} for i in range(pcm.shape[0])]
    else:
        raise ValueError(f"unknown input kind {src['kind']!r}")

    window_s = kwargs.get("window_seconds", 5.0)
    if sincnet and window_s is not None and abs(window_s - 5.0) > 1e-9:
        raise NotImplementedError("the SincNet path keeps the reference's fixed 5 s cuts")
    # ---- pieces the model sees: (recording index, start sample, length)
    pieces = []
    for ri, r in enumerate(recs):
        n = len(r["pcm"])
        if window_s is None:
            pieces.append((ri, 0, n))
        else:
            for st, ln in cut_into_windows(n, int(round(window_s * sr)), int(round(kwargs.get("min_window_seconds", 3.0) * sr))):
                pieces.append((ri, st, ln))
    W = None if window_s is None else int(round(window_s * sr))
    med_window = 0.02 if net.encoding_dim == 768 else 0.01   # vad_engine.py:207-208
    binarize = kwargs.get("binarize")   # None: threshold 0.5 + median as below; a dict in seconds (BINARIZE_DEFAULTS): uvad_binarize instead
    if binarize is not None:
        binarize = _binarize_frames(binarize, sincnet, frame_shift, sr)
    cuts = kwargs.get("cuts")   # None: every output below is what it was; a dict (CUTS_DEFAULTS): every result gains "cuts" (_attach_cuts)
    dev_labels = [None] * len(recs) if cuts is not None else None   # each recording's whole-row labels, kept on the device
    # None: nothing more; {recording_id: path or [(start_s, end_s, text)]}: every cut gains its supervisions / words and text, every result "audit"
    supervisions, alignments = kwargs.get("supervisions"), kwargs.get("alignments")
    if (supervisions is not None or alignments is not None) and cuts is None:
        raise ValueError("supervisions / alignments are joined with the cuts: pass cuts= as well")
    fuse = kwargs.get("fuse")   # None: one result per channel row, as ever; a dict (postprocess.fuse_config's mode / threshold / decide): one per file
    dev_probs = None
    if fuse is not None:
        from .postprocess import fuse_config
        if src["kind"] != "wav" or src.get("channels", "first") != "all":
            raise ValueError("fuse puts the channels of each file together: it needs input kind 'wav' with channels = 'all'")
        if set(fuse) - {"mode", "threshold", "decide"}:
            raise ValueError(f"unknown fuse option(s) {sorted(set(fuse) - {'mode', 'threshold', 'decide'})} (known: mode, threshold, decide; the groups are the files)")
        fuse = fuse_config(**fuse)
        dev_probs = [None] * len(recs)
    dev_best = None
    hop_s = kwargs.get("hop_seconds")
    if hop_s is not None:   # overlapping windows of window_seconds every hop_seconds, aggregated on the device; None: the cuts below, unchanged
        if window_s is None:
            raise ValueError("hop_seconds needs window_seconds (the window the model was trained on)")
        results = _predict_sliding(recs, net.runtime(device), sincnet, kwargs, window_s, hop_s, frame_shift, med_window, device, sr, dev_labels, binarize,
                                   dev_probs)
        if fuse is not None:
            results, recs, dev_labels, dev_best = _fuse_recordings(results, recs, dev_probs, net.runtime(device), fuse, binarize, sincnet, frame_shift,
                                                                   med_window, device, sr)
        if cuts is not None:
            _attach_cuts(results, recs, dev_labels, net.runtime(device), cuts, sincnet, frame_shift, device, int(kwargs["max_duration"] * sr), sr,
                         supervisions, alignments, dev_best)
        return _write_results(results, kwargs)

    # ---- batches: pieces of equal length together, at most max_duration seconds of audio per batch; with ragged_batches (whole
    #      recordings, window_seconds None) pieces of any length together, padded to the batch's longest, each row run on its own
    #      length (uvad_forward_lens; the SincNet model: uvad_forward_wav_lens, every norm over the row's own samples)
    ragged = bool(kwargs.get("ragged_batches", False)) and window_s is None
    order = sorted(range(len(pieces)), key=lambda i: (-pieces[i][2], i))
    batches, i = [], 0
    if ragged:
        batches = pack_ragged_batches([p[2] for p in pieces], int(kwargs["max_duration"] * sr))
        i = len(order)
    while i < len(order):
        n = pieces[order[i]][2]
        group = [order[i]]
        while (i + len(group) < len(order) and pieces[order[i + len(group)]][2] == n
               and (len(group) + 1) * n / float(sr) <= kwargs["max_duration"]):
            group.append(order[i + len(group)])
        i += len(group)
        batches.append(group)

    rt = net.runtime(device)
    pipe = None
    if len(batches) > 1:   # log-mel: kept tails (n < W) take the unfused branch below; SincNet: every batch, tails padded first
        pipe = open_pipeline(net, device, min(3, len(batches)))

    def piece_rows(group):   # int16 rows beside ingested f32 ones are read as q / 32768, the value the _i16 entry points give them
        rows = [recs[pieces[j][0]]["pcm"][pieces[j][1]:pieces[j][1] + pieces[j][2]] for j in group]
        if len({r.dtype for r in rows}) > 1:
            rows = [r.astype(np.float32) / np.float32(32768.0) if r.dtype == np.int16 else r for r in rows]
        return rows

    def stack(group):
        return torch.from_numpy(np.stack(piece_rows(group))).to(device)

    def stack_ragged(group):   # rows zero-padded to the longest (the padding is never read)
        rows = piece_rows(group)
        x = np.zeros((len(rows), max(len(r) for r in rows)), dtype=rows[0].dtype)
        for r, row in enumerate(rows):
            x[r, :len(row)] = row
        return torch.from_numpy(x).to(device)

    piece_probs = [None] * len(pieces)
    piece_post = {}   # ragged: piece -> (labels, intervals) from the batch's lens median and runs
    pending = []

    def ragged_post(group, probs):
        nsamp = [pieces[j][2] for j in group]
        fr = [rt.sincnet_num_frames(n) if sincnet else rt.num_frames(n) for n in nsamp]
        if binarize is not None:   # uvad_binarize in place of the median filter and the run walk
            lab, ivs = _binarize_post(rt, binarize, probs, fr, [n / sr for n in nsamp], sincnet, frame_shift)
        else:
            lab = median_filter(probs, window=med_window, lengths=fr)                      # uvad_median_filter_lens
            if sincnet:   # frame index -> seconds by the receptive field, as the dense path below (whole recordings: every frame is kept)
                ivs = [sincnet_labels_to_intervals(lab[r, :fr[r]], n / sr) if fr[r] else [] for r, n in enumerate(nsamp)]
            else:
                ivs = labels_to_intervals_batch(lab, frame_shift, runtime=rt, lengths=fr)     # uvad_label_runs_lens
        for r, j in enumerate(group):
            piece_probs[j] = probs[r, :fr[r]]
            piece_post[j] = (lab[r, :fr[r]], ivs[r])

    for group in batches:
        if ragged:
            x = stack_ragged(group)
            nsamp = [pieces[j][2] for j in group]
            if pipe is not None:
                pending.append((group, pipe.submit(x, want_logits=False, want_probs=True, lengths=nsamp)))
            else:
                fwd = rt.forward_wav if sincnet else rt.forward
                ragged_post(group, fwd(x, want_logits=False, lengths=nsamp)[1])
            continue
        n = pieces[group[0]][2]
        x = stack(group)
        if sincnet:   # (batch, samples), int16 from a wav file as it is (uvad_forward_wav_i16 reads q / 32768); the model consumes raw audio
            if W is not None and n < W:   # a kept tail: the recipe pads the AUDIO cut to the window (.pad(duration=5.0)), so every cut gives 293 frames
                xp = x.new_zeros((x.shape[0], W))   # (zero samples in either type)
                xp[:, :n] = x
                x = xp
            if pipe is not None:
                pending.append((group, pipe.submit(x, want_logits=False, want_probs=True)))
                continue
            probs = model(x.unsqueeze(1)).squeeze(-1)   # channel axis added as in vad_engine.py:252-255
        elif W is not None and n < W:
            # a kept tail (3 s < length < 5 s): features of the samples that exist, then lhotse's padding frames up to the
            # window's frame count, then the classifier (the reference pads FEATURES, not audio)
            feats = rt.fbank(x)
            T_full = rt.num_frames(W)
            padded = torch.full((feats.shape[0], T_full, feats.shape[2]), LOG_EPS_PAD, dtype=torch.float32, device=device)
            padded[:, :feats.shape[1]] = feats
            _, probs = rt.classify(padded, want_logits=False)
        elif pipe is not None:
            pending.append((group, pipe.submit(x, want_logits=False, want_probs=True)))
            continue
        else:
            _, probs = rt.forward(x, want_logits=False)          # fused PCM -> probabilities (uvad_forward / uvad_forward_i16)
        for r, j in enumerate(group):
            piece_probs[j] = probs[r]
    for group, p in pending:
        _, probs = p.result()
        if ragged:
            ragged_post(group, probs)
            continue
        for r, j in enumerate(group):
            piece_probs[j] = probs[r]
    if pipe is not None:
        pipe.close()

    # ---- labels per piece exactly as VadModel.predict_step derives them (vad_engine.py:204-211: threshold 0.5 + median
    #      filter per row), then the rows of a recording laid end to end (predict.py:451-458)
    results = []
    for ri, r in enumerate(recs):
        mine = [j for j in range(len(pieces)) if pieces[j][0] == ri]
        if not mine:
            results.append({"recording_id": r["id"], "num_frames": 0, "labels": np.zeros(0, np.uint8), "probs": np.zeros(0, np.float32),
                            "intervals": []})
            continue
        if ragged:   # one piece per recording, post-processed with its batch
            (j,) = mine
            labels, intervals = piece_post[j]
            results.append({"recording_id": r["id"], "num_frames": int(labels.shape[0]), "labels": labels.cpu().numpy().astype(np.uint8),
                            "probs": piece_probs[j].cpu().numpy(), "intervals": intervals})
            if dev_labels is not None:
                dev_labels[ri] = labels
            if dev_probs is not None:
                dev_probs[ri] = piece_probs[j]
            continue
        probs = torch.cat([piece_probs[j] for j in mine])
        duration = len(r["pcm"]) / sr
        # How many of a recording's frames are kept.  The reference lays the rows of ALL recordings end to end (preds_flat) and
        # gives recording i the slice [start_i, start_i + n_i) with start_i = the sum of the earlier n_j (predict.py:451-458,
        # predict_sincnet.py:330-336), n = ceil(duration / frame_shift) + 1 resp. ceil(get_num_frames(16000 * duration)) + 1.  A
        # recording's rows are whole padded windows, i.e. MORE than n frames (23.7 s -> 5 x 500 = 2500 rows vs n = 2371), so that
        # cumulative offset drifts: from the second recording on the reference's slice starts inside the previous recording's
        # rows.  That carry is DELIBERATELY NOT reproduced: every recording here keeps the first n frames of ITS OWN rows (what the
        # reference computes for the first recording, and for every recording of a one-recording run).  The per-recording
        # behaviour is pinned by tests (single recordings against the reference-generated fixture, two recordings against their
        # single-recording runs); parity with the reference's drifting multi-recording slices is unpinned by intent.
        keep = probs.shape[0]
        if sincnet:
            # n as the reference computes it: get_num_frames on the FLOAT 16000 * duration (receptive_field.py:28-55 floor-divides
            # whatever it is given), then ceil + 1
            keep = min(int(math.ceil(SincNet.num_frames(16000 * duration))) + 1, keep)
        elif window_s is not None:
            keep = min(int(math.ceil(duration / frame_shift)) + 1, keep)
        probs = probs[:keep]
        if binarize is not None:   # one uvad_binarize call on the recording's kept frames laid end to end: the state, the pauses and the
            # minimum durations carry across the windows' seams, which a per-window decision could not do
            lab, ivs = _binarize_post(rt, binarize, probs.reshape(1, -1).contiguous(), None, [duration], sincnet, frame_shift)
            labels, intervals = lab[0], ivs[0]
        else:
            by_len = {}
            for j in mine:
                by_len.setdefault(piece_probs[j].shape[0], []).append(j)
            lab_of = {}
            for T, js in by_len.items():
                lab = median_filter(torch.stack([piece_probs[j] for j in js]), window=med_window)   # (n, T) 0/1 on the GPU
                for k, j in enumerate(js):
                    lab_of[j] = lab[k]
            labels = torch.cat([lab_of[j] for j in mine])[:keep]
            if sincnet:   # :348-370 + :492-504: frame index -> seconds by receptive field (step 270 samples, offset round(0.5 * 991) = 496), NOT by frame_shift
                intervals = sincnet_labels_to_intervals(labels, duration)
            else:
                intervals = labels_to_intervals_batch(labels.unsqueeze(0), frame_shift)[0]   # run-length walk on the GPU (uvad_label_runs)
        results.append({"recording_id": r["id"], "num_frames": int(labels.shape[0]), "labels": labels.cpu().numpy().astype(np.uint8),
                        "probs": probs.cpu().numpy(), "intervals": intervals})
        if dev_labels is not None:
            dev_labels[ri] = labels
        if dev_probs is not None:
            dev_probs[ri] = probs
    if fuse is not None:
        results, recs, dev_labels, dev_best = _fuse_recordings(results, recs, dev_probs, rt, fuse, binarize, sincnet, frame_shift, med_window, device, sr)
    if cuts is not None:
        _attach_cuts(results, recs, dev_labels, rt, cuts, sincnet, frame_shift, device, int(kwargs["max_duration"] * sr), sr, supervisions, alignments,
                     dev_best)
    return _write_results(results, kwargs)


def _wav_duration(path: str) -> float:
    try:
        with wave.open(path, "rb") as w:
            return w.getnframes() / float(w.getframerate())
    except (wave.Error, EOFError):      # G.711 and the other forms read_audio takes
        raw, (_, _, rate) = read_audio(path)
        return raw.shape[0] / float(rate)


def test_vad(**kwargs):
    """The reference's test entry point (src/scripts/test.py:16-102, ``function == "test"``) with its lhotse / Lightning plumbing replaced
    by wav files and label files: ``input = {"kind": "wav", "paths": [...], "labels": [...]}``, one label file per recording in the
    ``start<TAB>end<TAB>LABEL`` text form the reference's get_audacity_labels writes.  The recordings go through predict_vad with every
    option it takes (window_seconds, hop_seconds, ragged_batches, ingest of telephone audio); then, on the device, the reference
    intervals are rasterised with the reference's rounding (postprocess.supervision_frames, uvad_intervals_to_labels) and two scoring
    states accumulate over all recordings as one ragged batch: predict_vad's OWN labels against the reference (the counts test_step
    logs, and per recording the FA / MD / DER fractions get_metrics averages, other_vad_metrics.py:204-255), and the raw probabilities
    (the loss and the threshold sweep).  Prints and returns {"metrics": the reference's test_* names pooled over all recordings,
    "recordings": [{recording_id, false_alarm, missed_detection, detection_error_rate}], "false_alarm" / "missed_detection" /
    "detection_error_rate": their means over the recordings, "det": postprocess.det_curve}."""
    from .postprocess import det_curve, read_label_file, score_metrics, supervision_frames
    src = kwargs["input"]
    if src.get("kind") != "wav" or len(src.get("labels", ())) != len(src["paths"]):
        raise ValueError('test_vad needs input = {"kind": "wav", "paths": [...], "labels": [one label file per path]}')
    if src.get("channels", "first") != "first" and kwargs.get("fuse") is None:   # with fuse= the channels are one recording again
        raise ValueError("test_vad scores one recording per file (channels = 'first')")
    sincnet = kwargs["feature_extractor"] == "sincnet"
    results = predict_vad(**kwargs)                        # sorted by recording id
    label_of = {os.path.basename(p): l for p, l in zip(src["paths"], src["labels"])}
    device = _resolve_device(kwargs["device"])
    from .postprocess import _shared_runtime
    rt = _shared_runtime(device)
    R, T = len(results), max(max(r["num_frames"] for r in results), 1)
    frames = [r["num_frames"] for r in results]
    probs = np.zeros((R, T), np.float32)
    labels = np.zeros((R, T), np.float32)
    tables = []
    for i, r in enumerate(results):
        probs[i, :frames[i]] = r["probs"]
        labels[i, :frames[i]] = r["labels"]
        duration = _wav_duration(next(p for p in src["paths"] if os.path.basename(p) == r["recording_id"]))
        tables.append(supervision_frames(read_label_file(label_of[r["recording_id"]]), duration, frame_shift=kwargs["frame_shift"],
                                         geometry="sincnet" if sincnet else "fbank", num_frames=frames[i]))
    max_iv = max(max(len(t) for t in tables), 1)
    iv = np.zeros((R, max_iv, 2), np.int32)
    for i, t in enumerate(tables):
        iv[i, :len(t)] = t
    lens = torch.tensor(frames, dtype=torch.int32, device=device)
    gt = rt.intervals_to_labels(iv, [len(t) for t in tables], T, lengths=lens)
    by_label = rt.score_open(points=[(0.5, 1)], bins=2)                                        # the labels as 0.0 / 1.0: exactly predict_vad's
    by_prob = rt.score_open(points=[(0.5, 1)], bins=int(kwargs.get("score_bins", 256)))        # the raw probabilities: loss and sweep
    rows = rt.score_step(by_label, torch.from_numpy(labels).to(device), gt, lengths=lens, rows=True).cpu().numpy()
    rt.score_step(by_prob, torch.from_numpy(probs).to(device), gt, lengths=lens)
    read_l, read_p = rt.score_read(by_label), rt.score_read(by_prob)
    metrics = score_metrics(read_l, prefix="test")
    metrics["test_loss"] = score_metrics(read_p, prefix="test")["test_loss"]
    recs = []
    for i, r in enumerate(results):
        n = max(frames[i], 1)
        fa, md = float(rows[i, 1]) / n, float(rows[i, 3]) / n
        recs.append({"recording_id": r["recording_id"], "false_alarm": fa, "missed_detection": md, "detection_error_rate": fa + md})
    out = {"metrics": metrics, "recordings": recs, "det": det_curve(read_p)}
    for k in ("false_alarm", "missed_detection", "detection_error_rate"):
        out[k] = float(np.mean([r[k] for r in recs])) if recs else 0.0
    for k, v in metrics.items():
        print(f"{k}: {v}")
    print(f"Detection Error Rate: {out['detection_error_rate']}\nFalse Alarm Rate: {out['false_alarm']}\n"
          f"Missed Detection Rate: {out['missed_detection']}")
    print(f"EER: {out['det']['eer']} at threshold {out['det']['eer_threshold']}; best threshold {out['det']['best_threshold']}")
    return out


def adapt_vad(**kwargs):
    """Head fine-tuning on wav files and label files in test_vad's formats (``function == "adapt"``): what the reference's training run
    (src/scripts/train.py with VadModel.training_step / configure_optimizers) does for the head alone.  ``input = {"kind": "wav", "paths":
    [...], "labels": [...], "val_paths": [...], "val_labels": [...]}``; without the held-out files the training files are validated on.
    Every recording is one batch of its own: its encoder output is computed once and cached (the LSTM stack is frozen), then
    ``max_epochs`` epochs of VadModel.adapt_head_step run over the cached taps (``accumulate_grad_batches`` calls per Adam step, lr =
    ``learning_rate``); every ``check_val_every_n_epoch`` epochs the head is committed and validation_step runs on the held-out files.
    Saves a Lightning-style checkpoint {"state_dict" (``model.`` keys), "epoch", "global_step"} to ``adapted_checkpoint_path`` (default:
    experiments_dir/adapted.ckpt) and returns {"train_loss": [per epoch], "val_loss": [(epoch, loss)], "val_metrics", "checkpoint_path"}.
    ``adapt_lstm_layers`` > 0: that many top LSTM layers learn as well (VadModel.adapt_step / adapt_commit); what is cached per recording
    is then the frozen prefix's output, the input of the lowest learning layer.  With them, train_vad's optimizer options apply
    (``gradient_clip_val``, ``weight_decay`` with ``adamw``, ``lr_schedule``, ``skip_nonfinite``: every step then ends in one
    uvad_optim_step), and the checkpoint carries "optimizer_states"; continuing an interrupted run is train_vad's."""
    from .postprocess import read_label_file, supervision_frames
    src = kwargs["input"]
    if src.get("kind") != "wav" or not src.get("paths") or len(src.get("labels", ())) != len(src["paths"]):
        raise ValueError('adapt_vad needs input = {"kind": "wav", "paths": [...], "labels": [one label file per path]}')
    val_paths, val_labels = list(src.get("val_paths") or src["paths"]), list(src.get("val_labels") or src["labels"])
    if len(val_paths) != len(val_labels):
        raise ValueError("adapt_vad needs one label file per held-out path")
    if kwargs["feature_extractor"] not in ("fbank", "sincnet"):
        raise NotImplementedError("feature_extractor must be 'fbank' or 'sincnet'")
    sincnet = kwargs["feature_extractor"] == "sincnet"
    torch.manual_seed(kwargs["seed"])
    device = _resolve_device(kwargs["device"])
    model_dict, sr = dict(kwargs["model_dict"]), 16000
    lr = float(kwargs.get("learning_rate", 1e-3))
    lstm_layers = int(kwargs.get("adapt_lstm_layers", 0) or 0)
    if kwargs["load_checkpoint"]:
        model = VadModel.load_from_checkpoint(checkpoint_path=kwargs["checkpoint_path"], model_name=kwargs["model_name"], model_dict=model_dict,
                                              learning_rate=lr)
    else:
        model = VadModel(model_name=kwargs["model_name"], model_dict=model_dict, learning_rate=lr)
        seed_weights(model.model, kwargs.get("weights_seed", 1234), kwargs.get("weights_scale", 4.0))
    model = model.to(device).eval()
    net = model.model
    if not sincnet:
        net.attach_fbank(FbankConfig(sampling_rate=sr, num_filters=net.encoding_dim, window_type=kwargs.get("window_type", "povey"),
                                     frame_shift=kwargs["frame_shift"], device="cuda"))
    rt = net.runtime(device)

    def batch_of(path, label_path, cache):
        pcm = torch.from_numpy(_wav_recordings(path, "first", rt, sr)[0]["pcm"]).to(device)[None]
        inputs = pcm if sincnet else rt.fbank(pcm)                  # (1, samples) for PyanNet, as _common_step takes them; (1, T, F) log-mel
        b = {"inputs": inputs}
        key = "lstm_in" if lstm_layers else "lstm_out"
        if cache:
            b[key] = (model.lstm_in(b, lstm_layers) if lstm_layers else model.lstm_out(b)).clone()
        T = b[key].shape[1] if cache else (net.num_frames(pcm.shape[1]) if sincnet else inputs.shape[1])
        table = supervision_frames(read_label_file(label_path), pcm.shape[1] / float(sr), frame_shift=kwargs["frame_shift"],
                                   geometry="sincnet" if sincnet else "fbank", num_frames=T)
        iv = np.zeros((1, max(len(table), 1), 2), np.int32)
        iv[0, :len(table)] = table
        b["is_voice"] = rt.intervals_to_labels(iv, [len(table)], T)
        return b

    train = [batch_of(p, l, True) for p, l in zip(src["paths"], src["labels"])]
    held = [batch_of(p, l, False) for p, l in zip(val_paths, val_labels)]
    epochs, every = int(kwargs.get("max_epochs", 10)), max(1, int(kwargs.get("check_val_every_n_epoch", 1)))
    accumulate = max(1, int(kwargs.get("accumulate_grad_batches", 1)))
    out = {"train_loss": [], "val_loss": [], "val_metrics": None}

    def validate(epoch):
        if epoch:                                                 # validation_step runs the context's head: serve the adapted one
            model.adapt_commit() if lstm_layers else model.adapt_head_commit()
        for i, b in enumerate(held):
            model.validation_step(b, i)
        out["val_metrics"] = model.validation_metrics(reset=True)
        out["val_loss"].append((epoch, out["val_metrics"]["val_loss"]))
        print(f"epoch {epoch}: val_loss {out['val_metrics']['val_loss']:.6f}")

    optim = _optim_options(kwargs, lr, epochs * len(train) // accumulate)
    if optim is not None and not lstm_layers:
        raise ValueError("adapt_vad: gradient_clip_val, weight_decay, lr_schedule and skip_nonfinite need adapt_lstm_layers > 0 (the joint "
                         "optimizer step runs in VadModel.adapt_step)")
    validate(0)
    step = 0
    for epoch in range(1, epochs + 1):
        if lstm_layers:
            losses = [model.adapt_step(b, i, accumulate=accumulate, lstm_layers=lstm_layers, optim=optim) for i, b in enumerate(train)]
        else:
            losses = [model.adapt_head_step(b, i, accumulate=accumulate) for i, b in enumerate(train)]
        step += len(train)
        out["train_loss"].append(float(torch.stack(losses).mean()))
        if epoch % every == 0 or epoch == epochs:
            validate(epoch)
    path = kwargs.get("adapted_checkpoint_path") or os.path.join(kwargs.get("experiments_dir", "."), "adapted.ckpt")
    if os.path.dirname(path):
        os.makedirs(os.path.dirname(path), exist_ok=True)
    blob = {"state_dict": {k: v.detach().cpu() for k, v in model.state_dict().items()}, "epoch": epochs, "global_step": step // accumulate}
    if lstm_layers:
        blob["optimizer_states"] = model.optimizer_state()
    torch.save(blob, path)
    out["checkpoint_path"] = path
    return out


def lr_schedule_table(schedule, base_lr: float, total_steps: int) -> np.ndarray:
    """The learning rate of every optimizer step t = 0 .. total_steps - 1 as a float64 array (uvad_optim_reset rounds the entries to f32):
    the table uvad_optim_step indexes with its count of applied steps.  schedule = None or {"name": ..., "warmup_steps": w (default 0), ...}:
      "constant"  base_lr;
      "warmup"    base_lr min(1, (t + 1) / w): torch's LambdaLR with that factor;
      "linear"    the warmup, then base_lr (1 - (1 - end_factor) (t - w) / (total_steps - w)), end_factor default 0;
      "cosine"    the warmup, then eta_min + (base_lr - eta_min) (1 + cos(pi (t - w) / (total_steps - w))) / 2: CosineAnnealingLR with
                  T_max = total_steps - w, eta_min default 0;
      "step"      the warmup times base_lr gamma^((t - w) // step_size): StepLR (gamma default 0.1).
    Every entry must come out finite and positive."""
    total = max(1, int(total_steps))
    sched = dict(schedule or {"name": "constant"})
    name, w = sched.get("name", "constant"), max(0, int(sched.get("warmup_steps", 0) or 0))
    if name not in ("constant", "warmup", "linear", "cosine", "step"):
        raise ValueError(f"lr_schedule: unknown name {name!r}")
    if name == "warmup" and w < 1:
        raise ValueError('lr_schedule "warmup" needs warmup_steps >= 1')
    base, out = float(base_lr), np.empty(total, np.float64)
    span = max(1, total - w)
    for t in range(total):
        if t < w:
            out[t] = base * min(1.0, (t + 1) / w)
        elif name in ("constant", "warmup"):
            out[t] = base
        elif name == "linear":
            out[t] = base * (1.0 - (1.0 - float(sched.get("end_factor", 0.0))) * (t - w) / span)
        elif name == "cosine":
            lo = float(sched.get("eta_min", 0.0))
            out[t] = lo + (base - lo) * (1.0 + math.cos(math.pi * (t - w) / span)) / 2.0
        else:
            out[t] = base * float(sched.get("gamma", 0.1)) ** ((t - w) // max(1, int(sched.get("step_size", 1))))
    if not (np.isfinite(out).all() and (out.astype(np.float32) > 0).all()):
        raise ValueError("lr_schedule: every learning rate must be finite and positive in f32")
    return out


def _optim_options(kwargs, lr: float, total_steps: int):
    """train_vad / adapt_vad's optimizer options -> the optim= dict of VadModel.train_step, or None when none is set (the run then ends
    every step in the _apply calls, as before the options existed)."""
    clip, wd = float(kwargs.get("gradient_clip_val") or 0.0), float(kwargs.get("weight_decay") or 0.0)
    sched, skip = kwargs.get("lr_schedule"), bool(kwargs.get("skip_nonfinite", False))
    if clip == 0.0 and wd == 0.0 and sched is None and not skip:
        return None
    return {"max_norm": clip, "weight_decay": wd, "adamw": bool(kwargs.get("adamw", False)), "skip_nonfinite": skip,
            "lr_table": [float(v) for v in lr_schedule_table(dict(sched) if sched is not None else None, lr, total_steps)]}


def _resume_point(kwargs, model):
    """With load_checkpoint and a checkpoint that carries "optimizer_states": hand them to the model (VadModel.load_optimizer_state) and
    -> (its epoch, its global_step): training continues from there.  Otherwise (0, 0): the checkpoint gives the weights only."""
    if not kwargs.get("load_checkpoint"):
        return 0, 0
    blob = torch.load(kwargs["checkpoint_path"], map_location="cpu", weights_only=True)
    if not isinstance(blob, dict) or blob.get("optimizer_states") is None:
        return 0, 0
    model.load_optimizer_state(blob["optimizer_states"])
    return int(blob.get("epoch", 0)), int(blob.get("global_step", 0))


def _wav_bank(paths, rt, sr, what):
    """The first channel of every file as f32 (through _wav_recordings, so other sample rates pass through the ingest stage); without
    files, one clip of one zero, for a stage that is switched off."""
    clips = [np.zeros(1, np.float32)] if not paths else []
    for p in paths:
        pcm = np.asarray(_wav_recordings(p, "first", rt, sr)[0]["pcm"])
        clips.append(pcm.astype(np.float32) * np.float32(1.0 / 32768.0) if pcm.dtype == np.int16 else pcm.astype(np.float32))
        if len(clips[-1]) < 1:
            raise ValueError(f"{p}: an empty {what} file")
    return clips


def _open_noise(kwargs, rt, seed, sr=16000):
    """train_vad's noise augmentation -> a mix state (VadRuntime.mix_open) or None.  ``noise`` = {"paths": [wav files], "snr": (10, 20),
    "mix_prob": 0.5, "snr_steps": 1024, "max_seg": 8, "seed": the run's}: what every training recipe of the reference does to its training
    phase (cuts.mix(noise_cuts, snr=(10, 20), mix_prob=0.5), src/datasets/*/utils.py), redrawn here for every batch on the device
    (uvad_mix_step).  Without ``noise``, ``enable_musan`` with ``musan["paths"]`` gives the same.  The files are read through
    _wav_recordings, so other sample rates pass through the ingest stage.  mix_prob = 0 needs no files: the stage runs and changes
    nothing."""
    noise = kwargs.get("noise")
    if noise is None and kwargs.get("enable_musan") and (kwargs.get("musan") or {}).get("paths"):
        noise = dict(kwargs["musan"])
    if noise is None:
        return None
    paths, mix_prob = list(noise.get("paths") or ()), float(noise.get("mix_prob", 0.5))
    if not paths and mix_prob != 0.0:
        raise ValueError('train_vad: noise needs "paths", a list of wav files')
    clips = _wav_bank(paths, rt, sr, "noise")
    return rt.mix_open(np.concatenate(clips), [len(c) for c in clips], snr=noise.get("snr", (10, 20)), mix_prob=mix_prob,
                       snr_steps=int(noise.get("snr_steps", 1024)), max_seg=int(noise.get("max_seg", 8)), seed=int(noise.get("seed", seed)))


def _open_reverb(kwargs, rt, seed, sr=16000):
    """train_vad's reverberation -> a reverb state (VadRuntime.reverb_open) or None.  ``reverb`` = {"paths": [wav files, one room impulse
    response each], "prob": 0.5, "normalize": True, "align": True, "max_seconds": None (a number: only that much of every response),
    "seed": the run's}: lhotse's reverb_rir, redrawn here for every batch on the device (uvad_reverb_step) in front of the noise mix.
    prob = 0 needs no files: the stage runs and changes nothing."""
    reverb = kwargs.get("reverb")
    if reverb is None:
        return None
    paths, prob = list(reverb.get("paths") or ()), float(reverb.get("prob", 0.5))
    if not paths and prob != 0.0:
        raise ValueError('train_vad: reverb needs "paths", a list of wav files')
    rirs = _wav_bank(paths, rt, sr, "impulse response")
    max_seconds = reverb.get("max_seconds")
    return rt.reverb_open(np.concatenate(rirs), [len(h) for h in rirs], prob=prob, normalize=bool(reverb.get("normalize", True)),
                          align=bool(reverb.get("align", True)), max_taps=0 if max_seconds is None else max(1, int(round(float(max_seconds) * sr))),
                          seed=int(reverb.get("seed", seed)))


def _augment(rt, reverb, mix, x, nsamp=None):
    """A stacked PCM batch through the augmentation chain, a fresh draw per batch: reverberation (into a new tensor: a row is read while
    it is written), then noise (in place).  -> the augmented batch"""
    if reverb is not None:
        x = rt.reverb_step(reverb, x, nsamp=nsamp)
    if mix is not None:
        rt.mix_step(mix, x, nsamp=nsamp, out=x)
    return x


def _save_training_checkpoint(kwargs, model, out, epoch: int, global_step: int, extra_states=None):
    """train_vad's checkpoint: {"state_dict", "epoch", "global_step", "optimizer_states" (VadModel.optimizer_state: every family's masters,
    m, v and scalars, and the joint optimizer's counts; extra_states, the device sampler's record, joins them)} at
    experiments_dir/checkpoint-epoch=NN.ckpt -> out, completed."""
    path = os.path.join(kwargs.get("experiments_dir", "."), f"checkpoint-epoch={epoch:02d}.ckpt")
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    out["global_step"] = global_step
    blob = {"state_dict": {k: v.detach().cpu() for k, v in model.state_dict().items()}, "epoch": epoch, "global_step": global_step}
    if getattr(model, "_adapt_full", None) is not None:
        blob["optimizer_states"] = model.optimizer_state()
        blob["optimizer_states"].update(extra_states or {})
    torch.save(blob, path)
    out["checkpoint_path"] = path
    return out


def sampler_corpus(paths, labels, rt, sr=16000):
    """Wav files and their label files -> what VadRuntime.sampler_open takes: (pcm back to back -- int16 when every file is, else f32 --,
    samples per recording, per recording the (n, 2) supervision table in samples, rounded to the nearest sample)."""
    from .postprocess import read_label_file
    pcms = [np.asarray(_wav_recordings(p, "first", rt, sr)[0]["pcm"]) for p in paths]
    if not all(x.dtype == np.int16 for x in pcms):
        pcms = [x.astype(np.float32) * np.float32(1.0 / 32768.0) if x.dtype == np.int16 else x.astype(np.float32) for x in pcms]
    sups = [np.array([(int(round(a * sr)), int(round(b * sr))) for a, b in read_label_file(l)], np.int64).reshape(-1, 2) for l in labels]
    return np.concatenate(pcms), [len(x) for x in pcms], sups


def _train_vad_device_sampler(kwargs, src, val_paths, val_labels, model, rt, device, seed, sr, sincnet):
    """train_vad with ``device_sampler=True``, for both front ends: the recordings and their supervision tables are uploaded once
    (sampler_corpus, VadRuntime.sampler_open) and every step is sampler_step -> _augment -> train_step; no batch is assembled on the host.
    Windows of ``window_seconds``; a tail is kept when it is longer than ``min_keep_seconds`` (default: 3 / 5 of the window for the waveform
    model, the reference's 3 s of 5 s, whose rows are zero-padded to the window, pad=True; for the log-mel model 0, raised to the longest
    tail that still has no frame).  ``input["datasets"]`` names each recording's dataset and ``dataset_weights`` = {name: weight} multiplexes
    them (the reference's dataset_weights; absent: one dataset).  An epoch is steps_per_epoch = (windows in all) // rows steps of
    rows = max_duration / window_seconds rows.  The sampler's record {draw ordinal, cursors} joins "optimizer_states" in the checkpoint
    (key "sampler"), so a resumed run draws the batches an uninterrupted one draws.  Validation walks the held-out recordings' windows in
    table order through a second state (shuffle=False)."""
    window_s = float(kwargs.get("window_seconds") or 5.0)
    Wn = int(round(window_s * sr))
    rows = max(1, int(float(kwargs["max_duration"]) / window_s))
    keep_s = kwargs.get("min_keep_seconds")
    keep = int(round((0.6 * window_s if sincnet else 0.0) * sr)) if keep_s is None else int(round(float(keep_s) * sr))
    if not sincnet:
        keep = max(keep, next(n for n in range(1, Wn + 1) if rt.num_frames(n) >= 1) - 1)      # every kept row has a frame
    geometry = "sincnet" if sincnet else "fbank"
    names = list(src.get("datasets") or ["all"] * len(src["paths"]))
    if len(names) != len(src["paths"]):
        raise ValueError('train_vad: input["datasets"] names one dataset per path')
    order = sorted(set(names), key=names.index)
    given = dict(kwargs.get("dataset_weights") or {})
    if set(given) - set(order):
        raise ValueError(f"train_vad: dataset_weights names unknown datasets {sorted(set(given) - set(order))}")
    weights = [float(given.get(n, 1.0)) for n in order]

    def open_state(paths, labels, **kw):
        pcm, lens, sups = sampler_corpus(paths, labels, rt, sr)
        st = rt.sampler_open(pcm, lens, sups, Wn, keep, geometry, pad=sincnet, seed=seed, **kw)
        return st, sum(n // Wn + (n % Wn > keep) for n in lens)

    st, n_windows = open_state(src["paths"], src["labels"], datasets=[order.index(n) for n in names], weights=weights, shuffle=True)
    held, n_held = open_state(val_paths, val_labels, shuffle=False)
    mix, reverb = _open_noise(kwargs, rt, seed, sr), _open_reverb(kwargs, rt, seed, sr)
    steps_per_epoch = max(1, n_windows // rows)
    epochs, every = int(kwargs.get("max_epochs", 10)), max(1, int(kwargs.get("check_val_every_n_epoch", 1)))
    accumulate = max(1, int(kwargs.get("accumulate_grad_batches", 1)))
    out = {"train_loss": [], "val_loss": [], "val_metrics": None, "steps_per_epoch": steps_per_epoch, "first_plan": None}

    def batch_of(res, augment):
        x = _augment(rt, reverb, mix, res["pcm"], res["nsamp"]) if augment else res["pcm"]
        if sincnet:
            return {"inputs": x, "is_voice": res["labels"]}
        return {"inputs": rt.fbank(x, lengths=res["nsamp"]), "is_voice": res["labels"], "lengths": res["frames"]}

    def validate(epoch):
        model.train_commit()
        for i, at in enumerate(range(0, n_held, rows)):               # table order from window 0, the last batch as short as it must be
            model.validation_step(batch_of(rt.sampler_step(held, min(rows, n_held - at), cursor=[at], draw=i), False), i)
        out["val_metrics"] = model.validation_metrics(reset=True)
        out["val_loss"].append((epoch, out["val_metrics"]["val_loss"]))
        print(f"epoch {epoch}: val_loss {out['val_metrics']['val_loss']:.6f}")

    optim = _optim_options(kwargs, float(kwargs.get("learning_rate", 1e-3)), epochs * steps_per_epoch // accumulate)
    first, done = _resume_point(kwargs, model)
    if first or done:
        record = torch.load(kwargs["checkpoint_path"], map_location="cpu", weights_only=True)["optimizer_states"].get("sampler")
        if record is None:
            raise ValueError("train_vad: the checkpoint was not written with device_sampler=True: it holds no sampler record")
        rt.sampler_write(st, np.asarray(record, np.int64))
    last = min(epochs, int(kwargs.get("stop_after_epoch") or epochs))
    step = done * accumulate
    for epoch in range(first + 1, last + 1):
        losses = []
        for _ in range(steps_per_epoch):
            res = rt.sampler_step(st, rows, plan=out["first_plan"] is None)
            if out["first_plan"] is None:
                out["first_plan"] = res["plan"].cpu().numpy().copy()
            losses.append(model.train_step(batch_of(res, True), step, accumulate=accumulate, optim=optim))
            step += 1
        out["train_loss"].append(float(torch.stack(losses).mean()))
        print(f"epoch {epoch}: train_loss {out['train_loss'][-1]:.6f}")
        if epoch % every == 0 or epoch == last:
            validate(epoch)
    return _save_training_checkpoint(kwargs, model, out, last, step // accumulate, {"sampler": [int(v) for v in rt.sampler_read(st)]})


def _train_vad_sincnet(kwargs, src, val_paths, val_labels, model, rt, device, seed, sr):
    """train_vad for the waveform PyanNet: each recording's waveform is cached on the device and cut into windows of ``window_seconds``;
    a window's labels are its own supervisions_feature_mask (supervision_frames, geometry "sincnet", over the window's own frames).
    The front end normalises over whole rows, so a batch holds rows of ONE length: full windows together, tails in batches of their
    own; a tail shorter than the receptive field (991 samples) has no frame and is skipped.  Shuffle, validation and the checkpoint are
    train_vad's.  With ``reverb`` / ``noise`` every stacked batch is reverberated, then mixed, on the device before its train_step
    (_augment); validation never is."""
    from .postprocess import read_label_file, supervision_frames
    net = model.model
    mix, reverb = _open_noise(kwargs, rt, seed, sr), _open_reverb(kwargs, rt, seed, sr)

    def labels_of(items, t0, n):
        """(1, T) labels of the n samples from t0 seconds on, from the recording's intervals."""
        T, dur = net.num_frames(n), n / float(sr)
        own = [(a - t0, b - t0) for a, b in items if b - t0 > 0 and a - t0 < dur]
        table = supervision_frames(own, dur, geometry="sincnet", num_frames=T)
        iv = np.zeros((1, max(len(table), 1), 2), np.int32)
        iv[0, :len(table)] = table
        return rt.intervals_to_labels(iv, [len(table)], T).clone()

    def recording(path, label_path):
        pcm = torch.from_numpy(np.array(_wav_recordings(path, "first", rt, sr)[0]["pcm"])).to(device)[None].float()
        if net.num_frames(pcm.shape[1]) < 1:
            raise ValueError(f"{path}: shorter than the receptive field (991 samples)")
        items = read_label_file(label_path)
        return {"inputs": pcm, "is_voice": labels_of(items, 0.0, pcm.shape[1]), "items": items}

    train = [recording(p, l) for p, l in zip(src["paths"], src["labels"])]
    held = train if (val_paths, val_labels) == (list(src["paths"]), list(src["labels"])) else [recording(p, l) for p, l in zip(val_paths, val_labels)]
    window_s = float(kwargs.get("window_seconds") or 5.0)
    Wn = max(991, int(round(window_s * sr)))
    windows, skipped = [], 0
    for r, b in enumerate(train):
        S = b["inputs"].shape[1]
        for s0 in range(0, S, Wn):
            n = min(Wn, S - s0)
            if net.num_frames(n) < 1:
                skipped += 1
                continue
            windows.append((r, s0, n, labels_of(b["items"], s0 / float(sr), n)))
    if skipped:
        print(f"train_vad: {skipped} tail window(s) shorter than the receptive field (991 samples) skipped")
    rows = max(1, int(float(kwargs["max_duration"]) / window_s))
    epochs, every = int(kwargs.get("max_epochs", 10)), max(1, int(kwargs.get("check_val_every_n_epoch", 1)))
    accumulate = max(1, int(kwargs.get("accumulate_grad_batches", 1)))
    out = {"train_loss": [], "val_loss": [], "val_metrics": None}

    def validate(epoch):
        model.train_commit()
        for i, b in enumerate(held):
            model.validation_step({"inputs": b["inputs"], "is_voice": b["is_voice"]}, i)
        out["val_metrics"] = model.validation_metrics(reset=True)
        out["val_loss"].append((epoch, out["val_metrics"]["val_loss"]))
        print(f"epoch {epoch}: val_loss {out['val_metrics']['val_loss']:.6f}")

    per_epoch = sum((sum(1 for w in windows if w[2] == n) + rows - 1) // rows for n in {w[2] for w in windows})
    optim = _optim_options(kwargs, float(kwargs.get("learning_rate", 1e-3)), epochs * per_epoch // accumulate)
    first, done = _resume_point(kwargs, model)
    last = min(epochs, int(kwargs.get("stop_after_epoch") or epochs))
    step = done * accumulate
    for epoch in range(first + 1, last + 1):
        order = torch.randperm(len(windows), generator=torch.Generator().manual_seed(seed + epoch)).tolist()
        by_len = {}
        for k in order:                                               # rows of one length per batch, in the shuffled order
            by_len.setdefault(windows[k][2], []).append(k)
        losses = []
        for n, ks in by_len.items():
            for i in range(0, len(ks), rows):
                picks = [windows[k] for k in ks[i:i + rows]]
                x = torch.stack([train[r]["inputs"][0, s0:s0 + n] for r, s0, _, _ in picks])
                y = torch.cat([lab for _, _, _, lab in picks])
                x = _augment(rt, reverb, mix, x)                      # a fresh draw per batch
                losses.append(model.train_step({"inputs": x, "is_voice": y}, step, accumulate=accumulate, optim=optim))
                step += 1
        out["train_loss"].append(float(torch.stack(losses).mean()))
        print(f"epoch {epoch}: train_loss {out['train_loss'][-1]:.6f}")
        if epoch % every == 0 or epoch == last:
            validate(epoch)
    return _save_training_checkpoint(kwargs, model, out, last, step // accumulate)


def train_vad(**kwargs):
    """Training from initialisation on wav files and label files in adapt_vad's ``input`` format (``function == "train"``): the
    accelerated form of the reference's src/scripts/train.py for ``feature_extractor = "fbank"`` (PyanNet2, below) and
    ``feature_extractor = "sincnet"`` with ``model_name = "PyanNet"`` (_train_vad_sincnet: waveform windows).  The PyanNet2 is built under
    ``torch.manual_seed(seed)`` -- torch's own initialisation, not seed_weights -- or loaded from ``checkpoint_path`` when
    ``load_checkpoint`` is set.  The log-mel features of every recording are computed once and cached, cut into windows of
    ``window_seconds`` (default 5.0; every tail is kept as a shorter row with its length), and batched up to ``max_duration`` seconds per
    batch; the window order is shuffled each epoch by a ``torch.Generator`` seeded with ``seed + epoch``.  Every batch is one
    VadModel.train_step: all LSTM layers and the head learn, with the dropout of ``model_dict["lstm"]["dropout"]`` (the reference's 0.5
    by default) between the LSTM layers, ``accumulate_grad_batches`` calls per Adam step, lr = ``learning_rate``.  With ``noise``
    (_open_noise) the PCM is cached instead of the features, windows are cut in samples, and every batch is mixed with noise on the
    device and framed with its rows' own lengths; ``reverb`` (_open_reverb) takes the same branch and reverberates every batch in front of
    the mix; ``noise = None`` and ``reverb = None`` launch what a run without the options launches.  Every
    ``check_val_every_n_epoch`` epochs (and after the last) the tensors are committed and validation_step runs on the held-out
    recordings (``input.val_paths``; the training files without them).  Saves a Lightning-style checkpoint {"state_dict" (``model.``
    keys), "epoch", "global_step", "optimizer_states"} to experiments_dir/checkpoint-epoch=NN.ckpt and returns {"train_loss": [per epoch],
    "val_loss": [(epoch, loss)], "val_metrics", "checkpoint_path", "global_step"}.
    Optimizer options (all off: every step ends in the three _apply calls and launches what it launched before they existed):
    ``gradient_clip_val`` (the global gradient norm over every learning tensor is clipped to it), ``weight_decay`` with ``adamw`` (False:
    L2 into the gradient; True: decoupled), ``lr_schedule`` (lr_schedule_table: a table over the run's epochs x batches // accumulate
    optimizer steps, built here and indexed on the device) and ``skip_nonfinite``; with any of them every step ends in one
    uvad_optim_step (VadModel.train_step's optim=).  ``stop_after_epoch`` ends the run early with that epoch's checkpoint.  With
    ``load_checkpoint`` and a checkpoint that carries "optimizer_states" the run CONTINUES: moments, step counts, bias corrections, the
    dropout draw ordinal and the optimizer's step index are restored and the epochs after the checkpoint's run, so that an interrupted
    run and an uninterrupted one end in the same bytes (with accumulate_grad_batches > 1 a partly accumulated step at the interruption
    is lost).  The draw ordinals of the noise mix and the reverberation are not part of the checkpoint: a resumed run with ``noise``
    or ``reverb`` draws others than an uninterrupted one.
    ``device_sampler=True`` (default False: everything above, launch for launch) draws the batches on the device instead
    (_train_vad_device_sampler: uvad_sampler_step in front of the same augmentation and train_step, weighted datasets, the sampler's
    record in the checkpoint); its window order is the sampler's own, not the torch.Generator's."""
    from .postprocess import read_label_file, supervision_frames
    src = kwargs["input"]
    if src.get("kind") != "wav" or not src.get("paths") or len(src.get("labels", ())) != len(src["paths"]):
        raise ValueError('train_vad needs input = {"kind": "wav", "paths": [...], "labels": [one label file per path]}')
    val_paths, val_labels = list(src.get("val_paths") or src["paths"]), list(src.get("val_labels") or src["labels"])
    if len(val_paths) != len(val_labels):
        raise ValueError("train_vad needs one label file per held-out path")
    if (kwargs["feature_extractor"], kwargs["model_name"]) not in (("fbank", "PyanNet2"), ("sincnet", "PyanNet")):
        raise NotImplementedError("train_vad trains a PyanNet2 on log-mel features (feature_extractor = 'fbank') or a PyanNet on the raw "
                                  "waveform (feature_extractor = 'sincnet')")
    sincnet = kwargs["feature_extractor"] == "sincnet"
    seed, sr = int(kwargs["seed"]), 16000
    torch.manual_seed(seed)
    device = _resolve_device(kwargs["device"])
    lr = float(kwargs.get("learning_rate", 1e-3))
    if kwargs["load_checkpoint"]:
        model = VadModel.load_from_checkpoint(checkpoint_path=kwargs["checkpoint_path"], model_name=kwargs["model_name"],
                                              model_dict=dict(kwargs["model_dict"]), learning_rate=lr)
    else:
        model = VadModel(model_name=kwargs["model_name"], model_dict=dict(kwargs["model_dict"]), learning_rate=lr)
    model = model.to(device).eval()      # the torch modules serve inference only; training runs in uvad_*_train_*
    net = model.model
    if not sincnet:
        net.attach_fbank(FbankConfig(sampling_rate=sr, num_filters=net.encoding_dim, window_type=kwargs.get("window_type", "povey"),
                                     frame_shift=kwargs["frame_shift"], device="cuda"))
    rt = net.runtime(device)
    if kwargs.get("device_sampler"):
        return _train_vad_device_sampler(kwargs, src, val_paths, val_labels, model, rt, device, seed, sr, sincnet)
    if sincnet:
        return _train_vad_sincnet(kwargs, src, val_paths, val_labels, model, rt, device, seed, sr)

    def recording(path, label_path):
        pcm = torch.from_numpy(_wav_recordings(path, "first", rt, sr)[0]["pcm"]).to(device)[None]
        feats = rt.fbank(pcm).clone()                                 # (1, T, F) log-mel, cached across the epochs
        T = feats.shape[1]
        table = supervision_frames(read_label_file(label_path), pcm.shape[1] / float(sr), frame_shift=kwargs["frame_shift"], geometry="fbank",
                                   num_frames=T)
        iv = np.zeros((1, max(len(table), 1), 2), np.int32)
        iv[0, :len(table)] = table
        return {"inputs": feats, "is_voice": rt.intervals_to_labels(iv, [len(table)], T).clone()}

    mix, reverb = _open_noise(kwargs, rt, seed, sr), _open_reverb(kwargs, rt, seed, sr)
    window_s = float(kwargs.get("window_seconds") or 5.0)
    rows = max(1, int(float(kwargs["max_duration"]) / window_s))
    epochs, every = int(kwargs.get("max_epochs", 10)), max(1, int(kwargs.get("check_val_every_n_epoch", 1)))
    accumulate = max(1, int(kwargs.get("accumulate_grad_batches", 1)))
    out = {"train_loss": [], "val_loss": [], "val_metrics": None}
    if mix is None and reverb is None:
        train = [recording(p, l) for p, l in zip(src["paths"], src["labels"])]
        held = train if (val_paths, val_labels) == (list(src["paths"]), list(src["labels"])) else [recording(p, l) for p, l in zip(val_paths, val_labels)]
        W = max(1, int(round(window_s / kwargs["frame_shift"])))
        windows = [(r, s, min(W, b["inputs"].shape[1] - s)) for r, b in enumerate(train) for s in range(0, b["inputs"].shape[1], W)]

        def batch_of(picks):
            """Rows of W frames, zero past each row's length (never read)."""
            x = torch.zeros((len(picks), W, net.encoding_dim), dtype=torch.float32, device=device)
            y = torch.zeros((len(picks), W), dtype=torch.uint8, device=device)
            for i, (r, s, n) in enumerate(picks):
                x[i, :n], y[i, :n] = train[r]["inputs"][0, s:s + n], train[r]["is_voice"][0, s:s + n]
            return {"inputs": x, "is_voice": y, "lengths": [n for _, _, n in picks]}
    else:
        # noise / reverb: the PCM is cached instead of the features, windows are cut in samples, and every batch is augmented (a fresh
        # draw), then framed with its rows' own lengths; a window's labels are computed over its own frames, as _train_vad_sincnet does
        def waveform(path, label_path):
            pcm = np.asarray(_wav_recordings(path, "first", rt, sr)[0]["pcm"])
            pcm = pcm.astype(np.float32) * np.float32(1.0 / 32768.0) if pcm.dtype == np.int16 else pcm.astype(np.float32)
            return {"pcm": torch.from_numpy(pcm).to(device), "items": read_label_file(label_path)}

        def labels_of(items, t0, n, T):
            dur = n / float(sr)
            own = [(a - t0, b - t0) for a, b in items if b - t0 > 0 and a - t0 < dur]
            table = supervision_frames(own, dur, frame_shift=kwargs["frame_shift"], geometry="fbank", num_frames=T)
            iv = np.zeros((1, max(len(table), 1), 2), np.int32)
            iv[0, :len(table)] = table
            return rt.intervals_to_labels(iv, [len(table)], T).clone()

        train = [waveform(p, l) for p, l in zip(src["paths"], src["labels"])]
        held = [recording(p, l) for p, l in zip(val_paths, val_labels)]      # validation is never mixed
        Wn = max(1, int(round(window_s * sr)))
        W = rt.num_frames(Wn)
        windows = []
        for r, b in enumerate(train):
            for s0 in range(0, b["pcm"].shape[0], Wn):
                n = min(Wn, b["pcm"].shape[0] - s0)
                T = rt.num_frames(n)
                if T >= 1:                                            # a tail without a frame is skipped
                    windows.append((r, s0, n, T, labels_of(b["items"], s0 / float(sr), n, T)))

        def batch_of(picks):
            """Rows of Wn samples, augmented on the device, then their log-mel features with each row's own length."""
            x = torch.zeros((len(picks), Wn), dtype=torch.float32, device=device)
            y = torch.zeros((len(picks), W), dtype=torch.uint8, device=device)
            for i, (r, s0, n, T, lab) in enumerate(picks):
                x[i, :n], y[i, :T] = train[r]["pcm"][s0:s0 + n], lab[0, :T]
            nsamp = [n for _, _, n, _, _ in picks]
            x = _augment(rt, reverb, mix, x, nsamp)
            return {"inputs": rt.fbank(x, lengths=nsamp), "is_voice": y, "lengths": [T for _, _, _, T, _ in picks]}

    def validate(epoch):
        model.train_commit()                                          # validation_step runs the context's tensors: serve the trained ones
        for i, b in enumerate(held):
            model.validation_step(b, i)
        out["val_metrics"] = model.validation_metrics(reset=True)
        out["val_loss"].append((epoch, out["val_metrics"]["val_loss"]))
        print(f"epoch {epoch}: val_loss {out['val_metrics']['val_loss']:.6f}")

    optim = _optim_options(kwargs, lr, epochs * ((len(windows) + rows - 1) // rows) // accumulate)
    first, done = _resume_point(kwargs, model)
    last = min(epochs, int(kwargs.get("stop_after_epoch") or epochs))
    step = done * accumulate
    for epoch in range(first + 1, last + 1):
        order = torch.randperm(len(windows), generator=torch.Generator().manual_seed(seed + epoch)).tolist()
        losses = []
        for i in range(0, len(order), rows):
            losses.append(model.train_step(batch_of([windows[k] for k in order[i:i + rows]]), step, accumulate=accumulate, optim=optim))
            step += 1
        out["train_loss"].append(float(torch.stack(losses).mean()))
        print(f"epoch {epoch}: train_loss {out['train_loss'][-1]:.6f}")
        if epoch % every == 0 or epoch == last:
            validate(epoch)
    return _save_training_checkpoint(kwargs, model, out, last, step // accumulate)
