"""VadRuntime: owns one ``uvad_ctx`` (device, model) and the device workspace; torch tensors are
used only as device-memory containers whose ``data_ptr()`` is handed to the C ABI together with
torch's current HIP stream.  Every method fails loudly if libuvad.so or the GPU is missing."""
import ctypes as C
import re
from typing import Dict, Optional

import numpy as np
import torch

from . import _lib
from .features import FbankConfig, make_mel_matrix, make_window
from .ingest import ENCODINGS, g711_table, ingest_plan, resample_ratio, resample_taps, stream_delay  # noqa: F401  (re-exported)


def _model_cfg(encoding_dim: int, lstm: dict, linear: dict, leaky_slope: float = 0.01) -> _lib.ModelCfg:
    return _lib.ModelCfg(int(encoding_dim), int(lstm["hidden_size"]), int(lstm["num_layers"]),
                         int(bool(lstm["bidirectional"])), int(linear.get("hidden_size", 128)),
                         int(linear.get("num_layers", 0)), float(leaky_slope))


def window_step_plan(samples: int, frames: int, chunk: int, window: int, lookahead: int, frame_len: int = 400, frame_shift: int = 160):
    """One step of a windowed stream group (uvad_window_step, include/uvad.h) from its counters (samples received, frames complete)
    -> (samples, frames, (k, window_lo, window_hi, emit_lo, emit_hi)) after the step.  Frame t spans samples
    [t * shift - n_left, t * shift - n_left + frame_len), n_left = (frame_len - shift) // 2; the model runs over frames
    [window_lo, window_hi) and the step emits frames [emit_lo, emit_hi), k = emit_hi - emit_lo of them."""
    n_left = (frame_len - frame_shift) // 2
    if samples == 0 and chunk < n_left:
        raise ValueError(f"the first chunk must hold at least (frame_len - shift) / 2 = {n_left} samples")
    if lookahead < 0 or lookahead + chunk // frame_shift + 1 > window:
        raise ValueError(f"need 0 <= lookahead and lookahead + chunk // frame_shift + 1 <= window (got {lookahead}, {chunk}, {window})")
    n = samples + chunk
    e = max(frames, (n + n_left - frame_len) // frame_shift + 1) if n + n_left - frame_len >= 0 else frames
    lo, hi = max(0, frames - lookahead), max(0, e - lookahead)
    return n, e, (hi - lo, max(0, e - window), e, lo, hi)


def window_schedule(steps: int, chunk: int, window: int, lookahead: int = 0, frame_len: int = 400, frame_shift: int = 160):
    """[(k, window_lo, window_hi, emit_lo, emit_hi)] for `steps` steps of `chunk` samples of a windowed stream group (window_step_plan)."""
    out, n, e = [], 0, 0
    for _ in range(steps):
        n, e, row = window_step_plan(n, e, chunk, window, lookahead, frame_len, frame_shift)
        out.append(row)
    return out


def wav_frame_geometry(stride: int = 10, kernel_size: int = 251, k2: int = 5, k3: int = 5):
    """(J, R) of a SincNet geometry (include/uvad.h): the frame step J = 27 * stride and the receptive field R, both in samples, of the
    three valid-padding (conv, MaxPool1d(3)) stages; frames(S) = 0 if S < R else (S - R) // J + 1.  The reference's: (270, 991)."""
    return 27 * stride, kernel_size + stride * (9 * k3 + 3 * k2 + 14)


def wav_window_step_plan(samples: int, frames: int, chunk: int, window: int, lookahead: int, J: int = 270, R: int = 991):
    """One step of a waveform window stream group (uvad_window_wav_step, include/uvad.h) from its counters (samples received, frames
    complete) -> (samples, frames, (k, window_lo, window_hi, emit_lo, emit_hi, sample_lo, sample_hi)) after the step.  The model runs
    over frames [window_lo, window_hi), i.e. samples [sample_lo, sample_hi), and the step emits frames [emit_lo, emit_hi), k of them."""
    kmax = -(-chunk // J)
    if lookahead < 0 or lookahead >= window:
        raise ValueError(f"need 0 <= lookahead < window (got lookahead {lookahead}, window {window})")
    if lookahead + kmax > window:
        raise ValueError(f"need lookahead + ceil(chunk / J) <= window (got {lookahead} + {kmax} > {window})")
    n = samples + chunk
    e = 0 if n < R else (n - R) // J + 1
    lo, hi = max(0, frames - lookahead), max(0, e - lookahead)
    w0 = max(0, e - window)
    s0 = J * w0
    return n, e, (hi - lo, w0, e, lo, hi, s0, s0 + (R + J * (e - w0 - 1) if e > w0 else 0))


def wav_window_schedule(steps: int, chunk: int, window: int, lookahead: int = 0, J: int = 270, R: int = 991):
    """[(k, window_lo, window_hi, emit_lo, emit_hi, sample_lo, sample_hi)] for `steps` steps of `chunk` samples of a waveform window
    stream group (wav_window_step_plan)."""
    out, n, e = [], 0, 0
    for _ in range(steps):
        n, e, row = wav_window_step_plan(n, e, chunk, window, lookahead, J, R)
        out.append(row)
    return out


def _slots_plan(flags, step_frames, window: int, lookahead: int):
    """Shared walk of a slot pool schedule: flags[step][slot] (bit 0 START, bit 1 END); step_frames(samples) -> frames complete after
    `samples` samples of a session.  -> [[(session, emit_lo, emit_hi, frames) per slot] per step]; session = -1 for an idle slot."""
    rows, sessions, live, next_id = [], {}, {}, 0
    for fl in flags:
        row = []
        for b, f in enumerate(fl):
            f = int(f)
            if f & 1:
                live[b] = next_id
                sessions[next_id] = [0, 0]
                next_id += 1
            sid = live.get(b)
            if sid is None:
                row.append((-1, 0, 0, 0))
                continue
            n_prev, e_prev = sessions[sid]
            n = n_prev + step_frames[1]
            e = max(e_prev, step_frames[0](n))
            lo = max(0, e_prev - lookahead)
            hi = e if f & 2 else max(0, e - lookahead)
            sessions[sid] = [n, e]
            row.append((sid, lo, hi, e))
            if f & 2:
                del live[b]
        rows.append(row)
    return rows


def window_slots_ld_out(chunk: int, lookahead: int, frame_shift: int = 160) -> int:
    """The least ld_out a log-mel slot pool step accepts: L + kmax, kmax = chunk // frame_shift + 1 frames a step can complete."""
    return lookahead + chunk // frame_shift + 1


def wav_window_slots_ld_out(chunk: int, lookahead: int, J: int = 270) -> int:
    """The least ld_out a waveform slot pool step accepts: L + kmax, kmax = ceil(chunk / J)."""
    return lookahead + -(-chunk // J)


def window_slots_plan(flags, chunk: int, window: int, lookahead: int = 0, frame_len: int = 400, frame_shift: int = 160):
    """The frames each step of a log-mel slot pool (uvad_window_slots_step, include/uvad.h) emits.  flags: per step, one flag per slot
    (bit 0 UVAD_SLOT_START, bit 1 UVAD_SLOT_END; a (steps, B) array or nested lists).  -> per step, per slot (session, emit_lo, emit_hi,
    frames): the slot's session (numbered in order of their starts, -1 for an idle slot), the session-local frames [emit_lo, emit_hi) the
    step emits (emit_hi - emit_lo = its count) and the session's complete frames after the step.  A session's frames are those of a
    single-feed window stream opened at its start (window_step_plan); its END step also flushes the lookahead frames held back."""
    n_left = (frame_len - frame_shift) // 2
    if chunk < n_left:
        raise ValueError(f"every step can be a session's first: chunk must hold at least (frame_len - shift) / 2 = {n_left} samples")
    if lookahead < 0 or lookahead >= window or window_slots_ld_out(chunk, lookahead, frame_shift) > window:
        raise ValueError(f"need 0 <= lookahead < window and lookahead + chunk // frame_shift + 1 <= window (got {lookahead}, {chunk}, {window})")

    def frames(n):
        return (n + n_left - frame_len) // frame_shift + 1 if n + n_left - frame_len >= 0 else 0

    return _slots_plan(flags, (frames, chunk), window, lookahead)


def wav_window_slots_plan(flags, chunk: int, window: int, lookahead: int = 0, J: int = 270, R: int = 991):
    """The frames each step of a waveform slot pool (uvad_window_wav_slots_step, include/uvad.h) emits: as window_slots_plan, with the
    whole frames of J samples and receptive field R of wav_window_step_plan."""
    if lookahead < 0 or lookahead >= window or wav_window_slots_ld_out(chunk, lookahead, J) > window:
        raise ValueError(f"need 0 <= lookahead < window and lookahead + ceil(chunk / J) <= window (got {lookahead}, {chunk}, {window})")
    return _slots_plan(flags, (lambda n: 0 if n < R else (n - R) // J + 1, chunk), window, lookahead)


STREAM_SLOTS_KMAX = 4       # LSTM_STACK_TMAX (csrc/uvad_internal.h): the frames a one-launch step takes


def stream_slots_kmax(chunk: int, frame_shift: int = 160) -> int:
    """The most frames a step of a causal stream's slot pool completes, and the least ld_out it accepts: ceil(chunk / frame_shift)
    (uvad_stream_slots_kmax)."""
    return -(-chunk // frame_shift)


def stream_slots_plan(flags, chunk: int, frame_len: int = 400, frame_shift: int = 160):
    """The frames each step of a causal stream's slot pool (uvad_stream_slots_step, include/uvad.h) emits, in closed form.  flags: per
    step, one flag per slot (bit 0 UVAD_SLOT_START, bit 1 UVAD_SLOT_END).  -> per step, per slot (session, emit_lo, emit_hi, frames) as
    window_slots_plan with lookahead 0: a frame is emitted in the step in which its last sample arrives, and the END step emits what its
    chunk completes and nothing more."""
    n_left = (frame_len - frame_shift) // 2
    if chunk < n_left:
        raise ValueError(f"every step can be a session's first: chunk must hold at least (frame_len - shift) / 2 = {n_left} samples")
    if stream_slots_kmax(chunk, frame_shift) > STREAM_SLOTS_KMAX:
        raise ValueError(f"a step completes up to ceil(chunk / frame_shift) = {stream_slots_kmax(chunk, frame_shift)} frames, the one-launch "
                         f"step takes {STREAM_SLOTS_KMAX}: chunk <= {STREAM_SLOTS_KMAX * frame_shift} samples")

    def frames(n):
        return (n + n_left - frame_len) // frame_shift + 1 if n + n_left - frame_len >= 0 else 0

    return _slots_plan(flags, (frames, chunk), 1, 0)


def sliding_count(frames: int, window: int, hop: int) -> int:
    """Windows that cover a recording of `frames` frames (uvad_sliding_count, include/uvad.h): 0 for an empty one, 1 up to a window's
    length, else ceil((frames - window) / hop) + 1: window j starts at frame j * hop and holds min(window, frames - j * hop) frames."""
    if frames < 0 or window < 1 or not 1 <= hop <= window:
        raise ValueError(f"need frames >= 0, window >= 1 and 1 <= hop <= window (got {frames}, {window}, {hop})")
    if frames == 0:
        return 0
    if frames <= window:
        return 1
    return -(-(frames - window) // hop) + 1


def sliding_plan(frames, window: int, hop: int):
    """The window list of the sliding calls from the recordings' frame counts: (counts, first) -- counts[r] = sliding_count(frames[r])
    and first, the R + 1 exclusive prefix sums the library takes as d_first (first[R] = N windows in all)."""
    counts = [sliding_count(int(t), window, hop) for t in frames]
    first = [0]
    for n in counts:
        first.append(first[-1] + n)
    return counts, first


class VadRuntime:
    def __init__(self, device, fbank: Optional[FbankConfig] = None, model: Optional[dict] = None, sincnet: Optional[dict] = None):
        """model: {"encoding_dim": int, "lstm": {...merged defaults...}, "linear": {...}} or None.
        sincnet: SincNet.config() (stride, n_filters, kernel_size, c2, k2, c3, k3, leaky_slope, eps) or None."""
        self.lib = _lib.load()
        dev = torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError(f"VadRuntime needs a GPU device, got {dev}; there is no CPU path")
        if not torch.cuda.is_available():
            raise RuntimeError("no HIP device visible to torch; libuvad has no CPU fallback")
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        self.device = dev
        self.fbank_cfg = fbank
        self.model_cfg = model
        fb_c = mc_c = None
        if fbank is not None:
            fb_c = _lib.FbankCfg(fbank.sampling_rate, fbank.frame_len_samples, fbank.frame_shift_samples, fbank.n_fft,
                                 fbank.num_filters, fbank.preemph_coeff, fbank.low_freq, fbank.high_freq,
                                 fbank.energy_floor, int(fbank.remove_dc_offset), int(fbank.snip_edges))
        if model is not None:
            mc_c = _model_cfg(model["encoding_dim"], model["lstm"], model["linear"], model.get("leaky_slope", 0.01))
        self._fb_c, self._mc_c = fb_c, mc_c
        self.ctx = C.c_void_p()
        code = self.lib.uvad_create(dev.index, C.byref(fb_c) if fb_c else None, C.byref(mc_c) if mc_c else None,
                                    C.byref(self.ctx))
        try:
            _lib.check(self.lib, self.ctx, code)
        except Exception:
            self.close()
            raise
        if fbank is not None:
            win = make_window(fbank.window_type, fbank.frame_len_samples)
            mel = make_mel_matrix(fbank.num_filters, fbank.n_fft, fbank.sampling_rate, fbank.low_freq,
                                  fbank.high_freq, fbank.norm_filters)
            self.set_tables(win, mel)
        self._ws = None
        self._finalized = False
        self._sn_c = None
        if sincnet is not None:
            self._sn_c = _lib.SincNetCfg(int(sincnet["stride"]), int(sincnet["n_filters"]), int(sincnet["kernel_size"]),
                                         int(sincnet["c2"]), int(sincnet["k2"]), int(sincnet["c3"]), int(sincnet["k3"]),
                                         float(sincnet.get("leaky_slope", 0.01)), float(sincnet.get("eps", 1e-5)))
            try:
                self._check(self.lib.uvad_sincnet_configure(self.ctx, C.byref(self._sn_c)))
            except Exception:
                self.close()
                raise

    # ------------------------------------------------------------------ setup
    def set_tables(self, window: np.ndarray, mel: np.ndarray):
        window = np.ascontiguousarray(window, np.float32)
        mel = np.ascontiguousarray(mel, np.float32)
        assert window.shape == (self._fb_c.frame_len,), window.shape
        assert mel.shape == (self._fb_c.n_mels, self._fb_c.n_fft // 2 + 1), mel.shape
        self._check(self.lib.uvad_set_tables(self.ctx, window.ctypes.data, mel.ctypes.data))

    def load_state_dict(self, sd: Dict[str, "torch.Tensor"]):
        """torch-keyed tensors (CPU or GPU; a Lightning ``model.`` prefix is accepted)."""
        for k, v in sd.items():
            if ".filterbank." in k and k.rsplit(".", 1)[1] not in ("low_hz_", "band_hz_", "window_", "n_"):
                continue   # inference runs the materialised bank, sent as "...conv1d.0.filters"; the band edges and the two buffers are
                           # what uvad_sincnet_train_reset builds the learning bank from
            a = np.ascontiguousarray(v.detach().to("cpu", torch.float32).numpy() if torch.is_tensor(v) else v, np.float32)
            shape = (C.c_int64 * a.ndim)(*a.shape)
            self._check(self.lib.uvad_set_weight(self.ctx, k.encode(), a.ctypes.data, shape, a.ndim))
        self._check(self.lib.uvad_finalize(self.ctx))
        self._finalized = True
        self._loaded_sd = dict(sd)       # references, not copies: lstm_train_input builds the frozen prefix's sibling context from them
        self._drop_lstm_prefix()
        self._weights_gen = getattr(self, "_weights_gen", 0) + 1   # uvad_finalize re-allocates every weight buffer: graphs captured before are stale

    def _drop_lstm_prefix(self):
        for rt in getattr(self, "_lstm_prefix", {}).values():
            rt.close()
        self._lstm_prefix = {}

    # ------------------------------------------------------------------ helpers
    def _check(self, code):
        _lib.check(self.lib, self.ctx, code)

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _dev_f32(self, t: "torch.Tensor", name: str) -> "torch.Tensor":
        if not torch.is_tensor(t) or t.device != self.device:
            raise RuntimeError(f"{name} must be a tensor on {self.device} (got {getattr(t, 'device', type(t))})")
        if t.dtype != torch.float32:
            t = t.float()
        return t.contiguous()

    def num_frames(self, S: int) -> int:
        return int(self.lib.uvad_num_frames(self.ctx, S))

    def _dev_lens(self, lengths, B: int, limit: int, dtype, what: str) -> "torch.Tensor":
        """Per-row lengths for a *_lens call: a tensor on this device (int32 / int64) is used as it is -- the library clamps it to
        [0, limit] on the device, so a captured graph can replay with new values -- anything else (a list, a CPU tensor) is validated
        here and uploaded."""
        if torch.is_tensor(lengths) and lengths.device == self.device:
            if lengths.dtype not in (torch.int32, torch.int64) or lengths.shape != (B,):
                raise ValueError(f"{what} must be an int32 / int64 tensor of shape ({B},), got {lengths.dtype} {tuple(lengths.shape)}")
            return lengths.to(dtype).contiguous()
        host = lengths.tolist() if torch.is_tensor(lengths) else list(lengths)
        if len(host) != B:
            raise ValueError(f"{what}: {len(host)} lengths for {B} rows")
        for v in host:
            if isinstance(v, bool) or int(v) != v or not 0 <= v <= limit:
                raise ValueError(f"{what}: every length must be an integer in [0, {limit}], got {v!r}")
        return torch.tensor([int(v) for v in host], dtype=dtype, device=self.device)

    def workspace(self, B: int, T: int) -> "torch.Tensor":
        need = int(self.lib.uvad_workspace_bytes(self.ctx, B, T))
        if self._ws is None or self._ws.numel() < need:
            self._ws = None
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._ws

    # ------------------------------------------------------------------ compute
    def fbank(self, pcm: "torch.Tensor", lengths=None) -> "torch.Tensor":
        """pcm (B,S) f32 or int16 on the GPU -> (B,T,n_mels) f32.  lengths: samples per row (B,); row b is framed as pcm[b, :lengths[b]]
        alone and its frames past uvad_num_frames(lengths[b]) are zero."""
        with torch.cuda.device(self.device):
            i16 = pcm.dtype == torch.int16
            if i16:
                if pcm.device != self.device:
                    raise RuntimeError(f"pcm must be on {self.device}")
                pcm = pcm.contiguous()
            else:
                pcm = self._dev_f32(pcm, "pcm")
            B, S = pcm.shape
            T = self.num_frames(S)
            feats = torch.empty((B, T, self._fb_c.n_mels), dtype=torch.float32, device=self.device)
            if lengths is None:
                fn = self.lib.uvad_fbank_i16 if i16 else self.lib.uvad_fbank
                self._check(fn(self.ctx, pcm.data_ptr(), B, S, feats.data_ptr(), self._stream()))
            else:
                n = self._dev_lens(lengths, B, S, torch.int64, "lengths (samples)")
                fn = self.lib.uvad_fbank_lens_i16 if i16 else self.lib.uvad_fbank_lens
                self._check(fn(self.ctx, pcm.data_ptr(), B, S, n.data_ptr(), feats.data_ptr(), self._stream()))
            return feats

    def classify(self, feats: "torch.Tensor", want_logits=True, want_probs=True, lengths=None):
        """feats (B,T,F) on the GPU -> (logits (B,T) | None, probs (B,T) | None).  lengths: valid frames per row (B,) -- pack_padded_sequence
        semantics: row b is the model on feats[b, :lengths[b]] alone, frames past it are never read and come out as 0."""
        with torch.cuda.device(self.device):
            feats = self._dev_f32(feats, "feats")
            B, T, F = feats.shape
            if F != self._mc_c.in_dim:
                raise ValueError(f"feature dim {F} != encoding_dim {self._mc_c.in_dim}")
            ws = self.workspace(B, T)
            logits = torch.empty((B, T), dtype=torch.float32, device=self.device) if want_logits else None
            probs = torch.empty((B, T), dtype=torch.float32, device=self.device) if want_probs else None
            if lengths is None:
                self._check(self.lib.uvad_classify(self.ctx, feats.data_ptr(), B, T,
                                                   logits.data_ptr() if want_logits else None,
                                                   probs.data_ptr() if want_probs else None,
                                                   ws.data_ptr(), ws.numel(), self._stream()))
            else:
                n = self._dev_lens(lengths, B, T, torch.int32, "lengths (frames)")
                self._check(self.lib.uvad_classify_lens(self.ctx, feats.data_ptr(), B, T, n.data_ptr(),
                                                        logits.data_ptr() if want_logits else None,
                                                        probs.data_ptr() if want_probs else None,
                                                        ws.data_ptr(), ws.numel(), self._stream()))
            self._last_bt = (B, T)
            return logits, probs

    def forward(self, pcm: "torch.Tensor", want_logits=True, want_probs=True, lengths=None):
        """pcm (B,S) f32 (or int16, as read from a wav file) on the GPU -> (logits, probs); features never leave the workspace.
        lengths: samples per row (B,); row b is the model on pcm[b, :lengths[b]] alone, its frames past uvad_num_frames(lengths[b]) are 0."""
        with torch.cuda.device(self.device):
            i16 = pcm.dtype == torch.int16
            if i16:
                if pcm.device != self.device:
                    raise RuntimeError(f"pcm must be on {self.device}")
                pcm = pcm.contiguous()
            else:
                pcm = self._dev_f32(pcm, "pcm")
            B, S = pcm.shape
            T = self.num_frames(S)
            ws = self.workspace(B, T)
            logits = torch.empty((B, T), dtype=torch.float32, device=self.device) if want_logits else None
            probs = torch.empty((B, T), dtype=torch.float32, device=self.device) if want_probs else None
            outs = (logits.data_ptr() if want_logits else None, probs.data_ptr() if want_probs else None, ws.data_ptr(), ws.numel(), self._stream())
            if lengths is None:
                fn = self.lib.uvad_forward_i16 if i16 else self.lib.uvad_forward
                self._check(fn(self.ctx, pcm.data_ptr(), B, S, *outs))
            else:
                n = self._dev_lens(lengths, B, S, torch.int64, "lengths (samples)")
                fn = self.lib.uvad_forward_lens_i16 if i16 else self.lib.uvad_forward_lens
                self._check(fn(self.ctx, pcm.data_ptr(), B, S, n.data_ptr(), *outs))
            self._last_bt = (B, T)
            return logits, probs

    # ------------------------------------------------------------------ SincNet front end (PyanNet)
    def sincnet_num_frames(self, S: int) -> int:
        return int(self.lib.uvad_sincnet_num_frames(self.ctx, S))

    def _wav_ws(self, B: int, S: int, T: int, with_classifier: bool) -> "torch.Tensor":
        need = int(self.lib.uvad_sincnet_workspace_bytes(self.ctx, B, S))
        if with_classifier:
            need += int(self.lib.uvad_workspace_bytes(self.ctx, B, T))
        if self._ws is None or self._ws.numel() < need:
            self._ws = None
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._ws

    def _dev_wav(self, wav: "torch.Tensor"):
        """(contiguous wav on the device, True if int16): int16 goes to the _i16 entries unconverted, anything else as f32."""
        if torch.is_tensor(wav) and wav.dtype == torch.int16:
            if wav.device != self.device:
                raise RuntimeError(f"wav must be a tensor on {self.device} (got {wav.device})")
            return wav.contiguous(), True
        return self._dev_f32(wav, "wav"), False

    def sincnet(self, wav: "torch.Tensor", lengths=None) -> "torch.Tensor":
        """wav (B,S) f32, or int16 as read from a wav file (samples read as q / 32768, the same signal as uvad_fbank_i16 / forward()
        take: the f32 call on q.float() / 32768 gives the same bits), on the GPU -> SincNet features (B, frames, c3).
        lengths: samples per row (B,); row b is SincNet on wav[b, :lengths[b]] alone (every norm over the row's own samples), its
        frames past sincnet_num_frames(lengths[b]) are 0 (uvad_sincnet_lens)."""
        if self._sn_c is None:
            raise RuntimeError("this runtime was created without a SincNet configuration")
        with torch.cuda.device(self.device):
            wav, i16 = self._dev_wav(wav)
            B, S = wav.shape
            T = self.sincnet_num_frames(S)
            if T <= 0:
                raise ValueError(f"{S} samples are too short for one SincNet frame")
            ws = self._wav_ws(B, S, T, False)
            feats = torch.empty((B, T, self._sn_c.c3), dtype=torch.float32, device=self.device)
            if lengths is None:
                fn = self.lib.uvad_sincnet_i16 if i16 else self.lib.uvad_sincnet
                self._check(fn(self.ctx, wav.data_ptr(), B, S, feats.data_ptr(), ws.data_ptr(), ws.numel(), self._stream()))
            else:
                n = self._dev_lens(lengths, B, S, torch.int64, "lengths (samples)")
                fn = self.lib.uvad_sincnet_lens_i16 if i16 else self.lib.uvad_sincnet_lens
                self._check(fn(self.ctx, wav.data_ptr(), B, S, n.data_ptr(), feats.data_ptr(), ws.data_ptr(), ws.numel(), self._stream()))
            return feats

    def forward_wav(self, wav: "torch.Tensor", want_logits=True, want_probs=True, lengths=None):
        """wav (B,S) f32, or int16 read as q / 32768 (as in sincnet()), on the GPU -> (logits, probs) of PyanNet (SincNet -> LSTM stack ->
        head); int16 runs uvad_forward_wav_i16.  lengths: samples per row (B,); row b is the model on wav[b, :lengths[b]] alone, its
        frames past sincnet_num_frames(lengths[b]) are 0 (uvad_forward_wav_lens)."""
        if self._sn_c is None:
            raise RuntimeError("this runtime was created without a SincNet configuration")
        with torch.cuda.device(self.device):
            wav, i16 = self._dev_wav(wav)
            B, S = wav.shape
            T = self.sincnet_num_frames(S)
            if T <= 0:
                raise ValueError(f"{S} samples are too short for one SincNet frame")
            ws = self._wav_ws(B, S, T, True)
            logits = torch.empty((B, T), dtype=torch.float32, device=self.device) if want_logits else None
            probs = torch.empty((B, T), dtype=torch.float32, device=self.device) if want_probs else None
            outs = (logits.data_ptr() if want_logits else None, probs.data_ptr() if want_probs else None, ws.data_ptr(), ws.numel(), self._stream())
            if lengths is None:
                fn = self.lib.uvad_forward_wav_i16 if i16 else self.lib.uvad_forward_wav
                self._check(fn(self.ctx, wav.data_ptr(), B, S, *outs))
            else:
                n = self._dev_lens(lengths, B, S, torch.int64, "lengths (samples)")
                fn = self.lib.uvad_forward_wav_lens_i16 if i16 else self.lib.uvad_forward_wav_lens
                self._check(fn(self.ctx, wav.data_ptr(), B, S, n.data_ptr(), *outs))
            self._last_bt = (B, T)
            return logits, probs

    def taps(self, lin: bool = True):
        """(lstm_out (B,T,H*D), lin_out (B,T,lin_hidden) | None) of the last classify/forward.  lin=False: the LSTM tap only (the
        feed-forward tap is not available in GEMM mode "f16p3" where the fused head ran: include/uvad.h)."""
        with torch.cuda.device(self.device):
            B, T = self._last_bt
            W = self._mc_c.hidden * (2 if self._mc_c.bidirectional else 1)
            y = torch.empty((B, T, W), dtype=torch.float32, device=self.device)
            z = None
            if lin and self._mc_c.lin_layers > 0:
                z = torch.empty((B, T, self._mc_c.lin_hidden), dtype=torch.float32, device=self.device)
            self._check(self.lib.uvad_get_taps(self.ctx, B, T, y.data_ptr(), z.data_ptr() if z is not None else None,
                                               self._ws.data_ptr(), self._stream()))
            return y, z

    def median_filter(self, probs: "torch.Tensor", kernel: int, lengths=None) -> "torch.Tensor":
        """lengths: valid frames per row (B,): the median of each row's prefix alone, labels past it 0."""
        with torch.cuda.device(self.device):
            probs = self._dev_f32(probs, "probs")
            B, T = probs.shape
            out = torch.empty((B, T), dtype=torch.uint8, device=self.device)
            if lengths is None:
                self._check(self.lib.uvad_median_filter(self.ctx, probs.data_ptr(), B, T, int(kernel), out.data_ptr(), self._stream()))
            else:
                n = self._dev_lens(lengths, B, T, torch.int32, "lengths (frames)")
                self._check(self.lib.uvad_median_filter_lens(self.ctx, probs.data_ptr(), B, T, n.data_ptr(), int(kernel), out.data_ptr(),
                                                             self._stream()))
            return out

    # ------------------------------------------------------------------ streaming (BASELINE cfg 5)
    def stream_open(self, B: int, chunk: int, graphs: bool = False):
        """Allocate and reset the carried state of B lock-step streams fed `chunk` samples per step.
        graphs: replay each distinct step shape as a hipGraph (see stream_step).  Off by default: a step of a causal 128-unit model
        is one launch (lstm_stack_kernel: feature stage, every layer and the head), 0.059 ms at BASELINE cfg 5 (512 feeds,
        20 ms chunks); a graph has nothing left to shorten (with the 14 per-layer launches of round 2 a replayed step took 0.133 ms
        against 0.125 ms enqueued kernel by kernel)."""
        with torch.cuda.device(self.device):
            nbytes = int(self.lib.uvad_stream_state_bytes(self.ctx, B))
            if nbytes == 0:
                raise RuntimeError("streaming needs a runtime built with both a FbankConfig and a model")
            state = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            ws = torch.empty(int(self.lib.uvad_stream_workspace_bytes(self.ctx, B, chunk)), dtype=torch.uint8, device=self.device)
            self._check(self.lib.uvad_stream_reset(self.ctx, state.data_ptr(), B, self._stream()))
            kmax = chunk // self._fb_c.frame_shift + 1
            return {"state": state, "ws": ws, "B": B, "chunk": chunk,
                    "out": torch.empty((B, kmax), dtype=torch.float32, device=self.device),
                    "in": torch.empty((B, chunk), dtype=torch.float32, device=self.device),
                    "graphs": {} if graphs else None, "weights_gen": getattr(self, "_weights_gen", 0)}

    def stream_step(self, st, pcm_chunk: "torch.Tensor") -> "torch.Tensor":
        """pcm_chunk (B, chunk) f32 on the GPU -> logits (B, k) of the k frames completed by this chunk (a view of a buffer that
        the next step overwrites).

        With stream_open(graphs=True): what a step enqueues depends on the stream group's host-side counters only through
        (k, offset, parity, first) (uvad_stream_peek), so the first step with a given combination is captured into a hipGraph
        while it is enqueued and later ones replay that graph and move the counters with uvad_stream_advance.  At the reference
        geometry (20 ms chunks, 10 ms shift) a group settles into two graphs."""
        with torch.cuda.device(self.device):
            pcm_chunk = self._dev_f32(pcm_chunk, "pcm_chunk")
            if tuple(pcm_chunk.shape) != (st["B"], st["chunk"]):
                raise ValueError(f"expected a ({st['B']}, {st['chunk']}) chunk, got {tuple(pcm_chunk.shape)}")
            out = st["out"]

            def enqueue(src):
                return self.lib.uvad_stream_step(self.ctx, src.data_ptr(), st["B"], st["chunk"], st["state"].data_ptr(),
                                                 out.data_ptr(), out.shape[1], st["ws"].data_ptr(), st["ws"].numel(), self._stream())

            graphs = st.get("graphs")
            if graphs is not None and st.get("weights_gen") != getattr(self, "_weights_gen", 0):
                graphs.clear()           # captured before a weight hot-swap: their kernel nodes point at freed buffers
                st["weights_gen"] = getattr(self, "_weights_gen", 0)
            if graphs is None:
                k = enqueue(pcm_chunk)
            else:
                kk, off, par, first = C.c_int(), C.c_int64(), C.c_int(), C.c_int()
                self._check(self.lib.uvad_stream_peek(self.ctx, st["state"].data_ptr(), st["chunk"], C.byref(kk), C.byref(off),
                                                      C.byref(par), C.byref(first)))
                key = (kk.value, off.value, par.value, first.value)
                st["in"].copy_(pcm_chunk)                    # the graphs read their input from a fixed buffer
                g = graphs.get(key)
                if g is None:
                    cur = torch.cuda.current_stream(self.device)
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g):                # capture: the step's launches are recorded, not run; its counters advance
                        k = enqueue(st["in"])
                    if k < 0:
                        self._check(k)
                    graphs[key] = g
                    torch.cuda.current_stream(self.device).wait_stream(cur)
                    g.replay()                               # now run it
                else:
                    g.replay()
                    k = self.lib.uvad_stream_advance(self.ctx, st["state"].data_ptr(), st["chunk"])
            if k < 0:
                self._check(k)
            return out[:, :k]

    # ------------------------------------------------------------------ windowed streaming (any model, bidirectional included)
    def _windowed_step(self, st, pcm_chunk, enqueue, peek, advance) -> int:
        """One step of a windowed stream group (uvad_window_step / uvad_window_wav_step): enqueue(src) runs the step on the chunk src.
        Without graphs, and during the warm-up (peek's replay key -1), the step is enqueued kernel by kernel; afterwards each replay
        key is captured once into a hipGraph reading the fixed buffer st["in"], replayed, and the host counters are moved by
        advance(ctx, state, chunk).  Graphs captured before a weight hot-swap are dropped.  Returns the step's k (checked)."""
        graphs = st.get("graphs")
        if graphs is not None and st.get("weights_gen") != getattr(self, "_weights_gen", 0):
            graphs.clear()           # captured before a weight hot-swap: their kernel nodes point at freed buffers
            st["weights_gen"] = getattr(self, "_weights_gen", 0)
        key = -1
        if graphs is not None:
            kk, rk = C.c_int(), C.c_int64()
            self._check(peek(self.ctx, st["state"].data_ptr(), st["chunk"], C.byref(kk), C.byref(rk)))
            key = rk.value
        if key < 0:
            k = enqueue(pcm_chunk)
        else:
            st["in"].copy_(pcm_chunk)                    # the graphs read their input from a fixed buffer
            g = graphs.get(key)
            if g is None:
                cur = torch.cuda.current_stream(self.device)
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):                # capture: the step's launches are recorded, not run; its counters advance
                    k = enqueue(st["in"])
                if k < 0:
                    self._check(k)
                graphs[key] = g
                torch.cuda.current_stream(self.device).wait_stream(cur)
                g.replay()                               # now run it
            else:
                g.replay()
                k = advance(self.ctx, st["state"].data_ptr(), st["chunk"])
        if k < 0:
            self._check(k)
        return k

    def window_stream_open(self, B: int, chunk: int, window: int = 500, lookahead: int = 0, graphs: bool = False):
        """Allocate and reset a windowed stream group (uvad_window_reset): B lock-step feeds of `chunk` samples per step, the model
        run from zero state over the last `window` frames, frames emitted `lookahead` frames behind the newest complete one.
        graphs: once the window is full, capture each distinct step (uvad_window_peek's replay key) into a hipGraph and replay it."""
        with torch.cuda.device(self.device):
            nbytes = int(self.lib.uvad_window_state_bytes(self.ctx, B, window))
            if nbytes == 0:
                raise RuntimeError("windowed streaming needs a runtime built with both a FbankConfig and a model, and window >= 1")
            state = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            self._check(self.lib.uvad_window_reset(self.ctx, state.data_ptr(), B, window, lookahead, self._stream()))
            ws = torch.empty(int(self.lib.uvad_window_workspace_bytes(self.ctx, B, chunk, window)), dtype=torch.uint8, device=self.device)
            kmax = chunk // self._fb_c.frame_shift + 1
            return {"state": state, "ws": ws, "B": B, "chunk": chunk, "window": window, "lookahead": lookahead, "samples": 0, "frames": 0,
                    "out": torch.empty((B, kmax), dtype=torch.float32, device=self.device),
                    "in": torch.empty((B, chunk), dtype=torch.float32, device=self.device),
                    "graphs": {} if graphs else None, "weights_gen": getattr(self, "_weights_gen", 0)}

    def window_stream_step(self, st, pcm_chunk: "torch.Tensor") -> "torch.Tensor":
        """pcm_chunk (B, chunk) f32 on the GPU -> logits (B, k) of the k frames this step emits (window_step_plan; a view of a buffer
        that the next step overwrites).  With window_stream_open(graphs=True) warm-up steps are enqueued kernel by kernel and the
        steady-state ones replay one hipGraph per replay key, then move the counters with uvad_window_advance."""
        with torch.cuda.device(self.device):
            pcm_chunk = self._dev_f32(pcm_chunk, "pcm_chunk")
            if tuple(pcm_chunk.shape) != (st["B"], st["chunk"]):
                raise ValueError(f"expected a ({st['B']}, {st['chunk']}) chunk, got {tuple(pcm_chunk.shape)}")
            n, e, (k_want, *_) = window_step_plan(st["samples"], st["frames"], st["chunk"], st["window"], st["lookahead"],
                                                  self._fb_c.frame_len, self._fb_c.frame_shift)
            out = st["out"]

            def enqueue(src):
                return self.lib.uvad_window_step(self.ctx, src.data_ptr(), st["B"], st["chunk"], st["state"].data_ptr(), out.data_ptr(),
                                                 None, out.shape[1], st["ws"].data_ptr(), st["ws"].numel(), self._stream())

            k = self._windowed_step(st, pcm_chunk, enqueue, self.lib.uvad_window_peek, self.lib.uvad_window_advance)
            if k != k_want:
                raise RuntimeError(f"uvad_window_step emitted {k} frames, the schedule says {k_want}")
            st["samples"], st["frames"] = n, e
            return out[:, :k]

    def window_features(self, st) -> "torch.Tensor":
        """The features (B, Tw, n_mels) of the window the last window_stream_step classified (debug tap, uvad_window_features)."""
        with torch.cuda.device(self.device):
            tw = C.c_int()
            self._check(self.lib.uvad_window_features(self.ctx, st["state"].data_ptr(), st["B"], None, C.byref(tw), self._stream()))
            feats = torch.empty((st["B"], tw.value, self._fb_c.n_mels), dtype=torch.float32, device=self.device)
            if tw.value:
                self._check(self.lib.uvad_window_features(self.ctx, st["state"].data_ptr(), st["B"], feats.data_ptr(), C.byref(tw),
                                                          self._stream()))
            return feats

    # ------------------------------------------------------------------ windowed streaming of the waveform model (PyanNet)
    def wav_window_geometry(self):
        """(J, R) of this runtime's SincNet: frame step and receptive field in samples (wav_frame_geometry)."""
        if self._sn_c is None:
            raise RuntimeError("this runtime was created without a SincNet configuration")
        q = self._sn_c
        return wav_frame_geometry(q.stride, q.kernel_size, q.k2, q.k3)

    def wav_window_stream_open(self, B: int, chunk: int, window: int = 293, lookahead: int = 0, graphs: bool = False,
                               dtype=torch.float32):
        """Allocate and reset a waveform window stream group (uvad_window_wav_reset): B lock-step feeds of `chunk` PCM samples per
        step (dtype torch.float32, or torch.int16 read as q / 32768), the model run from zero state over the last `window` frames,
        frames emitted `lookahead` frames behind the newest complete one.  graphs: once the window is full, capture each distinct step
        (uvad_window_wav_peek's replay key) into a hipGraph and replay it."""
        if dtype not in (torch.float32, torch.int16):
            raise ValueError(f"dtype must be torch.float32 or torch.int16, got {dtype}")
        J, R = self.wav_window_geometry()
        wav_window_step_plan(0, 0, chunk, window, lookahead, J, R)          # the limits, before anything is allocated
        i16 = int(dtype == torch.int16)
        with torch.cuda.device(self.device):
            nbytes = int(self.lib.uvad_window_wav_state_bytes(self.ctx, B, window, i16))
            if nbytes == 0:
                raise RuntimeError("waveform windowed streaming needs a runtime built with a model and a SincNet configuration")
            state = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            self._check(self.lib.uvad_window_wav_reset(self.ctx, state.data_ptr(), B, window, lookahead, i16, self._stream()))
            ws = torch.empty(int(self.lib.uvad_window_wav_workspace_bytes(self.ctx, B, chunk, window)), dtype=torch.uint8,
                             device=self.device)
            return {"state": state, "ws": ws, "B": B, "chunk": chunk, "window": window, "lookahead": lookahead, "J": J, "R": R,
                    "dtype": dtype, "samples": 0, "frames": 0,
                    "out": torch.empty((B, -(-chunk // J)), dtype=torch.float32, device=self.device),
                    "in": torch.empty((B, chunk), dtype=dtype, device=self.device),
                    "graphs": {} if graphs else None, "weights_gen": getattr(self, "_weights_gen", 0)}

    def wav_window_stream_step(self, st, pcm_chunk: "torch.Tensor") -> "torch.Tensor":
        """pcm_chunk (B, chunk) on the GPU, of the dtype the group was opened with -> logits (B, k) of the k frames this step emits
        (wav_window_step_plan; a view of a buffer that the next step overwrites).  With graphs=True warm-up steps are enqueued kernel by
        kernel and the steady-state ones replay one hipGraph per replay key, then move the counters with uvad_window_wav_advance."""
        with torch.cuda.device(self.device):
            if not torch.is_tensor(pcm_chunk) or pcm_chunk.device != self.device or pcm_chunk.dtype != st["dtype"]:
                raise RuntimeError(f"pcm_chunk must be a {st['dtype']} tensor on {self.device}")
            pcm_chunk = pcm_chunk.contiguous()
            if tuple(pcm_chunk.shape) != (st["B"], st["chunk"]):
                raise ValueError(f"expected a ({st['B']}, {st['chunk']}) chunk, got {tuple(pcm_chunk.shape)}")
            n, e, (k_want, *_) = wav_window_step_plan(st["samples"], st["frames"], st["chunk"], st["window"], st["lookahead"],
                                                      st["J"], st["R"])
            out = st["out"]
            fn = self.lib.uvad_window_wav_step_i16 if st["dtype"] == torch.int16 else self.lib.uvad_window_wav_step

            def enqueue(src):
                return fn(self.ctx, src.data_ptr(), st["B"], st["chunk"], st["state"].data_ptr(), out.data_ptr(), None, out.shape[1],
                          st["ws"].data_ptr(), st["ws"].numel(), self._stream())

            k = self._windowed_step(st, pcm_chunk, enqueue, self.lib.uvad_window_wav_peek, self.lib.uvad_window_wav_advance)
            if k != k_want:
                raise RuntimeError(f"uvad_window_wav_step emitted {k} frames, the schedule says {k_want}")
            st["samples"], st["frames"] = n, e
            return out[:, :k]

    def wav_window_features(self, st) -> "torch.Tensor":
        """The SincNet output (B, Tw, c3) of the window the model last ran on (debug tap, uvad_window_wav_features)."""
        with torch.cuda.device(self.device):
            tw = C.c_int()
            self._check(self.lib.uvad_window_wav_features(self.ctx, st["state"].data_ptr(), st["B"], None, C.byref(tw), self._stream()))
            feats = torch.empty((st["B"], tw.value, self._sn_c.c3), dtype=torch.float32, device=self.device)
            if tw.value:
                self._check(self.lib.uvad_window_wav_features(self.ctx, st["state"].data_ptr(), st["B"], feats.data_ptr(), C.byref(tw),
                                                              self._stream()))
            return feats

    # ------------------------------------------------------------------ slot pools: window streams whose feeds start and end independently
    def _slot_flags(self, B: int, start, end, buf=None):
        """start / end: None, a bool mask of B entries or a list of slot indices (host or device) -> uint8 flags [B] on the device
        (UVAD_SLOT_START | UVAD_SLOT_END), written into buf if given; None when neither is given and there is no buf."""
        if start is None and end is None and buf is None:
            return None

        def mask(m):
            if m is None:
                return torch.zeros(B, dtype=torch.uint8, device=self.device)
            t = m if torch.is_tensor(m) else torch.as_tensor(np.asarray(m))
            t = t.to(self.device)
            if t.dtype == torch.bool:
                if tuple(t.shape) != (B,):
                    raise ValueError(f"a slot mask must have {B} entries, got {tuple(t.shape)}")
                return t.to(torch.uint8)
            out = torch.zeros(B, dtype=torch.uint8, device=self.device)
            if t.numel():
                idx = t.reshape(-1).long()
                if not torch.is_tensor(m) and (int(idx.min()) < 0 or int(idx.max()) >= B):
                    raise ValueError(f"slot indices must lie in [0, {B})")
                out[idx] = 1
            return out

        flags = mask(start) | (mask(end) << 1)
        if buf is None:
            return flags
        buf.copy_(flags)
        return buf

    def _slots_step(self, st, pcm_chunk, start, end, fn):
        """One slot pool step: eager, or (graphs=True) the single graph captured on the first step and replayed for every later one,
        reading the chunk and the flags from fixed buffers.  Graphs captured before a weight hot-swap are dropped."""
        B = st["B"]
        out, counts = st["out"], st["counts"]
        ep = st.get("endpoint")
        fz = st.get("fuse")
        if fz is not None and getattr(self, "_fuse_current", None) is not fz:
            self._fuse_configure(fz)                 # another fusion state was used on this runtime since: the context holds one
            if st["graphs"] is not None:
                st["graph"] = None                   # ... and a captured node names the arrays of the configuration it was captured with

        def enqueue(src, flags):
            fp = flags.data_ptr() if flags is not None else None
            r = fn(self.ctx, src.data_ptr(), fp, B, st["chunk"], st["state"].data_ptr(), out.data_ptr(),
                   st["probs"].data_ptr() if "probs" in st else None, out.shape[1], counts.data_ptr(), st["ws"].data_ptr(), st["ws"].numel(),
                   self._stream())
            p_ptr, c_ptr, f_ptr = st["probs"].data_ptr() if "probs" in st else None, counts.data_ptr(), fp
            if r == 0 and fz is not None:            # the fusion right behind the pool step: one row per group for whatever follows
                r = self._fuse_enqueue(fz, p_ptr, out.shape[1], B, out.shape[1], c_ptr, fp, False, True)
                p_ptr, c_ptr, f_ptr = fz["fused"].data_ptr(), fz["glens"].data_ptr(), fz["flags"].data_ptr() if fp is not None else None
            if r == 0 and ep is not None:            # the endpointer right behind: probabilities, counts and flags as they are
                step = self._endpoint_hyst_enqueue if "lag" in ep else self._endpoint_enqueue
                r = step(ep, p_ptr, c_ptr, f_ptr)
            if r == 0 and st.get("gate") is not None:   # ... and the gate behind it: the pool's chunk, the endpointer's labels, the same flags
                r = self._gate_enqueue(st["gate"], src.data_ptr(), ep["labels"].data_ptr(), ep["lab_counts"].data_ptr(), fp)
            if r == 0 and st.get("group_gate") is not None:   # ... or the group gate: the pool's chunk, the fusion's best bytes, group lengths
                # and OR-ed flags, the endpointer's labels, and the rows' own flag bytes for the lockstep check
                r = self._gate_group_enqueue(st["group_gate"], src.data_ptr(), B, fz["best"].data_ptr(), fz["best"].shape[1], fz["glens"].data_ptr(),
                                             ep["labels"].data_ptr(), ep["lab_counts"].data_ptr(), f_ptr, fp)
            return r

        if st["graphs"] is None:
            self._check(enqueue(pcm_chunk, self._slot_flags(B, start, end)))
            return out, counts
        if st.get("weights_gen") != getattr(self, "_weights_gen", 0):
            st["graph"] = None       # captured before a weight hot-swap: its kernel nodes point at freed buffers
            st["weights_gen"] = getattr(self, "_weights_gen", 0)
        st["in"].copy_(pcm_chunk)
        self._slot_flags(B, start, end, st["flags"])
        if st["graph"] is None:
            cur = torch.cuda.current_stream(self.device)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):                    # capture: recorded, not run
                r = enqueue(st["in"], st["flags"])
            self._check(r)
            st["graph"] = g
            st["graphs"] += 1
            torch.cuda.current_stream(self.device).wait_stream(cur)
        st["graph"].replay()
        return out, counts

    _ENDPOINT_KEYS = {"kernel", "pad", "threshold"}
    _ENDPOINT_HYST_KEYS = {"onset", "offset", "min_on", "min_off", "pad_on", "pad_off"}

    def _slots_fuse(self, st, fuse, gate):
        """fuse: None or {"groups": [[slots of one stream's channels], ...], "mode", "threshold", "decide", "weights"} (fuse_open's).  One
        more node of the pool's step -- inside the one capture under graphs=True -- between the pool step and the endpointer: the
        pool's probabilities, counts and flag bytes go through uvad_fuse, and the endpointer (if any) is opened for the G groups and reads
        the fused rows, the group counts and the OR-ed flags.  st["fuse"] holds fused / glens / best / flags, overwritten by the next
        step, and stats, accumulated over the steps (fuse_read).  The members of a group must be stepped in lockstep: the same START /
        END flags and so the same counts every step -- which holds for the channels of one stream through ingest_step.  Opening or using
        another fusion state on this runtime re-configures the context: the pool configures it back at its next step.  gate= behind a
        fused pool is refused (the mono gate has no channel choice per fragment): group_gate= (_slots_group_gate) is the gate of a fused pool."""
        if fuse is None:
            return None
        if gate is not None:
            raise ValueError("gate= together with fuse= is not built: the gate would need a channel choice per fragment")
        from .postprocess import fuse_config
        fuse = dict(fuse)
        if fuse.get("groups") is None:
            raise ValueError("fuse needs groups: the slots of each stream's channels")
        q = fuse_config(**fuse)
        if max(max(g) for g in q["groups"]) >= st["B"]:
            raise ValueError(f"fuse groups name a slot at or past the pool's {st['B']}")
        fz = self.fuse_open(fuse.pop("groups"), **fuse)
        ld = st["out"].shape[1]
        self._fuse_buffers(fz, ld, False, True, True)
        need = int(self.lib.uvad_fuse_ws_bytes(self.ctx, st["B"], ld))
        fz["ws"] = torch.zeros(max(need, 16), dtype=torch.uint8, device=self.device)
        return fz

    def _slots_endpoint(self, st, endpoint, gate=None, geometry=None, fuse=None, group_gate=None):
        """endpoint: None, {"kernel", "pad", "threshold"} (any subset) for the median endpointer (endpoint_open), or {"onset", "offset",
        "min_on", "min_off", "pad_on", "pad_off"} (any non-empty subset; binarize_config's dict as it is) for the hysteresis endpointer
        (endpoint_hyst_open).  The pool gets a probabilities buffer and an endpointer over its B slots whose step is enqueued right behind
        every pool step -- inside the one capture under graphs=True -- with the pool's counts and flags.  st["endpoint"] holds its events /
        ev_counts / active, overwritten by the next step."""
        fz = self._slots_fuse(st, fuse, gate)
        if fz is not None:
            st["fuse"] = fz
            st["probs"] = torch.zeros_like(st["out"])
        if endpoint is None:
            if gate is not None:
                raise ValueError("gate needs an endpoint: the gate reads the labels an endpointer finalises")
            return st
        keys = set(endpoint)
        hyst = keys & self._ENDPOINT_HYST_KEYS
        if hyst and keys & self._ENDPOINT_KEYS:
            raise ValueError(f"endpoint parameters mix the median endpointer's {sorted(keys & self._ENDPOINT_KEYS)} with the hysteresis "
                             f"endpointer's {sorted(hyst)}: give one set")
        extra = keys - (self._ENDPOINT_HYST_KEYS if hyst else self._ENDPOINT_KEYS)
        if extra:
            raise ValueError(f"unknown endpoint parameters {sorted(extra)} " +
                             ("(onset, offset, min_on, min_off, pad_on, pad_off)" if hyst else "(kernel, pad, threshold)"))
        st["probs"] = st["probs"] if "probs" in st else torch.zeros_like(st["out"])
        st["endpoint"] = (self.endpoint_hyst_open if hyst else self.endpoint_open)(fz["G"] if fz is not None else st["B"], st["out"].shape[1],
                                                                                  **endpoint)
        if gate is not None:
            st["gate"] = self._slots_gate(st, dict(gate), geometry)
        if group_gate is not None:
            st["group_gate"] = self._slots_group_gate(st, group_gate, geometry)
        return st

    def _slots_group_gate(self, st, group_gate, geometry):
        """group_gate: {"decide_frames": D, ...} with any of _slots_gate's keys and best_history (postprocess.group_gate_config).  The gate
        of a fused pool (gate_group_open): per group and step the speech audio of the group's cuts, each cut whole from the member that
        won most of its first D frames.  hop / lead / tail default to the pool's geometry, lag_frames as _slots_gate computes it, the two
        histories to the derived ones.  Its step is enqueued behind the endpointer's -- inside the one capture under graphs=True -- on
        the pool's input buffer, the fusion's best bytes, group lengths and OR-ed flags, the endpointer's labels and counts, and the
        pool's flag bytes (the lockstep check).  st["group_gate"] holds out / seg / seg_counts, overwritten by the next step
        (gate_group_collect reads them)."""
        from .postprocess import group_gate_config
        q = group_gate_config(group_gate, st.get("fuse"), st.get("endpoint"))
        hop, lead, tail = geometry
        ep = st["endpoint"]
        ep_lag = ep["lag"] if "lag" in ep else ep["kernel"] // 2
        q.setdefault("hop", hop)
        q.setdefault("lead", lead)
        q.setdefault("tail", tail)
        lag = q.pop("lag_frames", st["lookahead"] + ep_lag + -(-tail // hop))
        return self.gate_group_open(st["fuse"], st["chunk"], ep["labels"].shape[1], st["in"].dtype, lag, q.pop("decide_frames"), **q)

    def _slots_gate(self, st, gate, geometry):
        """gate: {} or any of pad, max_len, hop, lead, tail, lag_frames, history, ld_out, max_seg (gate_open's).  geometry = (hop, lead,
        tail) of the pool's frames: frame t spans samples [t hop - lead, (t + 1) hop + tail), and hop / lead / tail default to it, so a
        cut holds every sample its frames saw and no record is SHORT.  lag_frames defaults to the pool's lookahead + the endpointer's lag
        (kernel // 2, or uvad_endpoint_hyst_lag) + ceil(tail / hop), the frames a complete frame trails the newest sample by.  pad
        defaults to 0: the hysteresis endpointer's labels are already padded (pad_on / pad_off), and the median endpointer's pad shapes
        its events, not its labels -- give pad here to widen the cuts as its events are widened.  The gate's step is enqueued behind the
        endpointer's -- inside the one capture under graphs=True -- on the pool's input chunk, the endpointer's labels and the pool's flags;
        st["gate"] holds its out / seg / seg_counts, overwritten by the next step (gate_collect reads them)."""
        hop, lead, tail = geometry
        ep = st["endpoint"]
        ep_lag = ep["lag"] if "lag" in ep else ep["kernel"] // 2
        gate.setdefault("hop", hop)
        gate.setdefault("lead", lead)
        gate.setdefault("tail", tail)
        lag = gate.pop("lag_frames", st["lookahead"] + ep_lag + -(-tail // hop))
        return self.gate_open(st["B"], st["chunk"], ep["labels"].shape[1], st["in"].dtype, lag, **gate)

    def window_slots_open(self, B: int, chunk: int, window: int = 500, lookahead: int = 0, graphs: bool = False, endpoint=None, gate=None,
                          fuse=None, group_gate=None):
        """Allocate and reset a log-mel slot pool (uvad_window_slots_reset): B slots stepping `chunk` samples at a time, each holding at
        most one session, windows of `window` frames, frames emitted `lookahead` frames behind the newest complete one (the END step
        flushes them).  graphs: capture the first step into a hipGraph and replay it for every later step.  endpoint: _slots_endpoint;
        gate (needs endpoint): _slots_gate; fuse: _slots_fuse (the endpointer then serves the groups, not the slots); group_gate (needs
        fuse and endpoint): _slots_group_gate."""
        if group_gate is not None:
            from .postprocess import group_gate_config
            group_gate_config(group_gate, fuse, endpoint)                    # refused before anything is allocated
        window_slots_plan([], chunk, window, lookahead, self._fb_c.frame_len, self._fb_c.frame_shift)   # the limits, before allocating
        n_left = (self._fb_c.frame_len - self._fb_c.frame_shift) // 2
        with torch.cuda.device(self.device):
            nbytes = int(self.lib.uvad_window_slots_state_bytes(self.ctx, B, window))
            if nbytes == 0:
                raise RuntimeError("slot pools need a runtime built with both a FbankConfig and a model, and window >= 1")
            state = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            self._check(self.lib.uvad_window_slots_reset(self.ctx, state.data_ptr(), B, chunk, window, lookahead, self._stream()))
            ws = torch.empty(int(self.lib.uvad_window_slots_workspace_bytes(self.ctx, B, chunk, window)), dtype=torch.uint8, device=self.device)
            ld = window_slots_ld_out(chunk, lookahead, self._fb_c.frame_shift)
            return self._slots_endpoint(
                {"state": state, "ws": ws, "B": B, "chunk": chunk, "window": window, "lookahead": lookahead,
                 "out": torch.empty((B, ld), dtype=torch.float32, device=self.device),
                 "counts": torch.zeros(B, dtype=torch.int32, device=self.device),
                 "in": torch.empty((B, chunk), dtype=torch.float32, device=self.device),
                 "flags": torch.zeros(B, dtype=torch.uint8, device=self.device),
                 "graphs": 0 if graphs else None, "graph": None, "weights_gen": getattr(self, "_weights_gen", 0)}, endpoint, gate,
                (self._fb_c.frame_shift, n_left, self._fb_c.frame_len - self._fb_c.frame_shift - n_left), fuse, group_gate)

    def window_slots_step(self, st, pcm_chunk: "torch.Tensor", start=None, end=None):
        """pcm_chunk (B, chunk) f32 on the GPU; start / end: slots whose session starts with this chunk / ends after it (bool masks or
        index lists, host or device).  -> (logits (B, lookahead + kmax), counts int32 (B,)), both on the device and overwritten by the
        next step: row b holds the counts[b] frames slot b emits this step in its first columns (window_slots_plan says which)."""
        with torch.cuda.device(self.device):
            pcm_chunk = self._dev_f32(pcm_chunk, "pcm_chunk")
            if tuple(pcm_chunk.shape) != (st["B"], st["chunk"]):
                raise ValueError(f"expected a ({st['B']}, {st['chunk']}) chunk, got {tuple(pcm_chunk.shape)}")
            return self._slots_step(st, pcm_chunk, start, end, self.lib.uvad_window_slots_step)

    def window_slots_features(self, st):
        """(features (B, W, n_mels), Tw int32 (B,)): the window each slot's last step classified, left-aligned (uvad_window_slots_features)."""
        with torch.cuda.device(self.device):
            feats = torch.empty((st["B"], st["window"], self._fb_c.n_mels), dtype=torch.float32, device=self.device)
            tw = torch.empty(st["B"], dtype=torch.int32, device=self.device)
            self._check(self.lib.uvad_window_slots_features(self.ctx, st["state"].data_ptr(), st["B"], feats.data_ptr(), tw.data_ptr(),
                                                            self._stream()))
            return feats, tw

    def wav_window_slots_open(self, B: int, chunk: int, window: int = 293, lookahead: int = 0, graphs: bool = False,
                              dtype=torch.float32, endpoint=None, gate=None, fuse=None, group_gate=None):
        """Allocate and reset a waveform slot pool (uvad_window_wav_slots_reset): window_slots_open for the SincNet PyanNet, samples of
        dtype torch.float32 or torch.int16 (read as q / 32768).  endpoint: _slots_endpoint; gate (needs endpoint): _slots_gate; fuse:
        _slots_fuse; group_gate (needs fuse and endpoint): _slots_group_gate."""
        if group_gate is not None:
            from .postprocess import group_gate_config
            group_gate_config(group_gate, fuse, endpoint)                    # refused before anything is allocated
        if dtype not in (torch.float32, torch.int16):
            raise ValueError(f"dtype must be torch.float32 or torch.int16, got {dtype}")
        J, R = self.wav_window_geometry()
        wav_window_slots_plan([], chunk, window, lookahead, J, R)            # the limits, before anything is allocated
        i16 = int(dtype == torch.int16)
        with torch.cuda.device(self.device):
            nbytes = int(self.lib.uvad_window_wav_slots_state_bytes(self.ctx, B, window, i16))
            if nbytes == 0:
                raise RuntimeError("waveform slot pools need a runtime built with a model and a SincNet configuration")
            state = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            self._check(self.lib.uvad_window_wav_slots_reset(self.ctx, state.data_ptr(), B, chunk, window, lookahead, i16, self._stream()))
            ws = torch.empty(int(self.lib.uvad_window_wav_slots_workspace_bytes(self.ctx, B, chunk, window)), dtype=torch.uint8,
                             device=self.device)
            return self._slots_endpoint(
                {"state": state, "ws": ws, "B": B, "chunk": chunk, "window": window, "lookahead": lookahead, "J": J, "R": R,
                 "dtype": dtype,
                 "out": torch.empty((B, wav_window_slots_ld_out(chunk, lookahead, J)), dtype=torch.float32, device=self.device),
                 "counts": torch.zeros(B, dtype=torch.int32, device=self.device),
                 "in": torch.empty((B, chunk), dtype=dtype, device=self.device),
                 "flags": torch.zeros(B, dtype=torch.uint8, device=self.device),
                 "graphs": 0 if graphs else None, "graph": None, "weights_gen": getattr(self, "_weights_gen", 0)}, endpoint, gate,
                (J, 0, R - J), fuse, group_gate)

    def wav_window_slots_step(self, st, pcm_chunk: "torch.Tensor", start=None, end=None):
        """window_slots_step for a waveform slot pool: pcm_chunk (B, chunk) of the dtype the pool was opened with."""
        with torch.cuda.device(self.device):
            if not torch.is_tensor(pcm_chunk) or pcm_chunk.device != self.device or pcm_chunk.dtype != st["dtype"]:
                raise RuntimeError(f"pcm_chunk must be a {st['dtype']} tensor on {self.device}")
            pcm_chunk = pcm_chunk.contiguous()
            if tuple(pcm_chunk.shape) != (st["B"], st["chunk"]):
                raise ValueError(f"expected a ({st['B']}, {st['chunk']}) chunk, got {tuple(pcm_chunk.shape)}")
            fn = self.lib.uvad_window_wav_slots_step_i16 if st["dtype"] == torch.int16 else self.lib.uvad_window_wav_slots_step
            return self._slots_step(st, pcm_chunk, start, end, fn)

    def wav_window_slots_features(self, st):
        """(SincNet output (B, W, c3), Tw int32 (B,)) of each slot's last step (uvad_window_wav_slots_features)."""
        with torch.cuda.device(self.device):
            feats = torch.empty((st["B"], st["window"], self._sn_c.c3), dtype=torch.float32, device=self.device)
            tw = torch.empty(st["B"], dtype=torch.int32, device=self.device)
            self._check(self.lib.uvad_window_wav_slots_features(self.ctx, st["state"].data_ptr(), st["B"], feats.data_ptr(), tw.data_ptr(),
                                                                self._stream()))
            return feats, tw

    # ------------------------------------------------------------------ the causal stream's slot pool (uvad_stream_slots_*)
    def stream_slots_open(self, B: int, chunk: int, graphs: bool = False, endpoint=None, gate=None, fuse=None, group_gate=None):
        """Allocate and reset a slot pool of the causal streaming step (uvad_stream_slots_reset): B slots stepping `chunk` samples at a
        time, each holding at most one session, one launch per step.  The pool exists where stream_step is one launch (a causal model with
        128 hidden units, 64 or 80 features, up to 8 layers, a 128-wide head; chunks of up to 4 frame shifts): anything else raises.
        graphs: capture the first step into a hipGraph and replay it for every later step.  endpoint / gate / fuse / group_gate: as
        window_slots_open, with lookahead 0.  The outputs are stream_slots_kmax(chunk) columns wide."""
        if group_gate is not None:
            from .postprocess import group_gate_config
            group_gate_config(group_gate, fuse, endpoint)                    # refused before anything is allocated
        stream_slots_plan([], chunk, self._fb_c.frame_len, self._fb_c.frame_shift)   # the limits, before allocating
        n_left = (self._fb_c.frame_len - self._fb_c.frame_shift) // 2
        with torch.cuda.device(self.device):
            nbytes = int(self.lib.uvad_stream_slots_state_bytes(self.ctx, B))
            if nbytes == 0:
                raise RuntimeError("slot pools need a runtime built with both a FbankConfig and a model")
            state = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            self._check(self.lib.uvad_stream_slots_reset(self.ctx, state.data_ptr(), B, chunk, self._stream()))
            ws = torch.empty(int(self.lib.uvad_stream_slots_workspace_bytes(self.ctx, B, chunk)), dtype=torch.uint8, device=self.device)
            ld = stream_slots_kmax(chunk, self._fb_c.frame_shift)
            return self._slots_endpoint(
                {"state": state, "ws": ws, "B": B, "chunk": chunk, "lookahead": 0,
                 "out": torch.empty((B, ld), dtype=torch.float32, device=self.device),
                 "counts": torch.zeros(B, dtype=torch.int32, device=self.device),
                 "in": torch.empty((B, chunk), dtype=torch.float32, device=self.device),
                 "flags": torch.zeros(B, dtype=torch.uint8, device=self.device),
                 "graphs": 0 if graphs else None, "graph": None, "weights_gen": getattr(self, "_weights_gen", 0)}, endpoint, gate,
                (self._fb_c.frame_shift, n_left, self._fb_c.frame_len - self._fb_c.frame_shift - n_left), fuse, group_gate)

    def stream_slots_step(self, st, pcm_chunk: "torch.Tensor", start=None, end=None):
        """pcm_chunk (B, chunk) f32 on the GPU; start / end as window_slots_step.  -> (logits (B, kmax), counts int32 (B,)), both on the
        device and overwritten by the next step: row b holds the counts[b] frames slot b completes with this chunk in its first columns
        (stream_slots_plan says which).  There is no peek / advance: under graphs=True every step replays the one captured graph."""
        with torch.cuda.device(self.device):
            pcm_chunk = self._dev_f32(pcm_chunk, "pcm_chunk")
            if tuple(pcm_chunk.shape) != (st["B"], st["chunk"]):
                raise ValueError(f"expected a ({st['B']}, {st['chunk']}) chunk, got {tuple(pcm_chunk.shape)}")
            return self._slots_step(st, pcm_chunk, start, end, self.lib.uvad_stream_slots_step)

    # ------------------------------------------------------------------ live endpointing (uvad_endpoint_*)
    def endpoint_open(self, B: int, ld_in: int, kernel: int = 25, pad: int = 0, threshold: float = 0.5, max_events=None):
        """Allocate and reset an endpointer of B slots (uvad_endpoint_reset): per slot the streaming median of `kernel` taps at `threshold`,
        its runs widened by `pad` frames and merged, reported as START / END events.  ld_in: columns of the probability rows a step
        reads; max_events: events kept per slot and step (default ld_in + kernel // 2 + 2, which never overflows)."""
        cfg = _lib.EndpointCfg(int(kernel), int(pad), float(threshold))
        if B < 1 or ld_in < 1:
            raise ValueError(f"need B >= 1 and ld_in >= 1, got {B}, {ld_in}")
        h = int(kernel) // 2
        max_events = ld_in + h + 2 if max_events is None else int(max_events)
        if max_events < 0:
            raise ValueError("max_events must be >= 0")
        with torch.cuda.device(self.device):
            nbytes = int(self.lib.uvad_endpoint_state_bytes(self.ctx, B, C.byref(cfg)))
            if nbytes == 0:
                raise ValueError(f"bad endpoint configuration: kernel {kernel} (odd, 1 .. 255), pad {pad} (0 .. 2^20), threshold {threshold} (finite)")
            state = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            self._check(self.lib.uvad_endpoint_reset(self.ctx, state.data_ptr(), nbytes, B, C.byref(cfg), self._stream()))
            return {"state": state, "B": B, "ld_in": ld_in, "kernel": int(kernel), "pad": int(pad), "threshold": float(threshold),
                    "max_events": max_events,
                    "events": torch.zeros((B, max_events, 2), dtype=torch.int32, device=self.device),
                    "ev_counts": torch.zeros(B, dtype=torch.int32, device=self.device),
                    "active": torch.zeros(B, dtype=torch.uint8, device=self.device),
                    "labels": torch.zeros((B, ld_in + h), dtype=torch.uint8, device=self.device),
                    "lab_counts": torch.zeros(B, dtype=torch.int32, device=self.device)}

    def _endpoint_enqueue(self, ep, probs_ptr, counts_ptr, flags_ptr, fn=None):
        """fn: the step to enqueue, uvad_endpoint_step or (same argument list) uvad_endpoint_hyst_step."""
        return (fn or self.lib.uvad_endpoint_step)(self.ctx, probs_ptr, ep["ld_in"], counts_ptr, flags_ptr, ep["B"], ep["state"].data_ptr(),
                                                   ep["state"].numel(), ep["events"].data_ptr() if ep["max_events"] else None,
                                                   ep["max_events"], ep["ev_counts"].data_ptr(), ep["active"].data_ptr(),
                                                   ep["labels"].data_ptr(), ep["labels"].shape[1], ep["lab_counts"].data_ptr(), self._stream())

    def endpoint_step(self, ep, probs: "torch.Tensor", counts: "torch.Tensor", start=None, end=None):
        """probs (B, ld_in) f32 and counts (B,) int32 on the GPU: slot b consumes probs[b, :counts[b]]; start / end as window_slots_step.
        -> (events (B, max_events, 2) int32 {kind 1 START / 2 END, frame}, ev_counts (B,) int32, active (B,) uint8), on the device and
        overwritten by the next step; ep["labels"] / ep["lab_counts"] hold the labels the step finalised."""
        return self._endpoint_run(ep, self._endpoint_enqueue, probs, counts, start, end)

    def _endpoint_run(self, ep, enqueue, probs, counts, start, end):
        """One eager step of either endpointer: the checks on probs and counts, the flag byte, then `enqueue`."""
        with torch.cuda.device(self.device):
            probs = self._dev_f32(probs, "probs")
            if tuple(probs.shape) != (ep["B"], ep["ld_in"]):
                raise ValueError(f"expected ({ep['B']}, {ep['ld_in']}) probabilities, got {tuple(probs.shape)}")
            if not torch.is_tensor(counts) or counts.device != self.device or counts.dtype != torch.int32 or tuple(counts.shape) != (ep["B"],):
                raise ValueError(f"counts must be an int32 tensor of shape ({ep['B']},) on {self.device}")
            flags = self._slot_flags(ep["B"], start, end)
            self._check(enqueue(ep, probs.data_ptr(), counts.contiguous().data_ptr(), flags.data_ptr() if flags is not None else None))
            return ep["events"], ep["ev_counts"], ep["active"]

    # ------------------------------------------------------------------ live hysteresis endpointing (uvad_endpoint_hyst_*)
    def endpoint_hyst_open(self, B: int, ld_in: int, onset: float = 0.5, offset=None, min_on: int = 0, min_off: int = 0, pad_on: int = 0,
                           pad_off: int = 0, max_events=None):
        """Allocate and reset a hysteresis endpointer of B slots (uvad_endpoint_hyst_reset): per slot the decisions of `binarize` -- on at
        !(p < onset), off at p < offset (default: onset), intervals shorter than min_on frames dropped, pauses shorter than min_off
        filled, pad_on / pad_off frames added -- reported as START / END events the moment they are certain.  The dict has endpoint_open's
        shape, plus "lag": its labels buffer is ld_in + lag columns wide.  max_events: events kept per slot and step (default ld_in + 1,
        which never overflows)."""
        cfg = _lib.BinarizeCfg(float(onset), float(onset if offset is None else offset), int(min_on), int(min_off), int(pad_on), int(pad_off))
        if B < 1 or ld_in < 1:
            raise ValueError(f"need B >= 1 and ld_in >= 1, got {B}, {ld_in}")
        max_events = ld_in + 1 if max_events is None else int(max_events)
        if max_events < 0:
            raise ValueError("max_events must be >= 0")
        with torch.cuda.device(self.device):
            nbytes = int(self.lib.uvad_endpoint_hyst_state_bytes(self.ctx, B, C.byref(cfg)))
            lag = int(self.lib.uvad_endpoint_hyst_lag(C.byref(cfg)))
            if nbytes == 0 or lag < 0:
                raise ValueError(f"bad hysteresis configuration: onset {cfg.onset} and offset {cfg.offset} (finite, offset <= onset), min_on "
                                 f"{min_on}, min_off {min_off}, pad_on {pad_on}, pad_off {pad_off} (0 .. 2^20)")
            state = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            self._check(self.lib.uvad_endpoint_hyst_reset(self.ctx, state.data_ptr(), nbytes, B, C.byref(cfg), self._stream()))
            return {"state": state, "B": B, "ld_in": ld_in, "onset": cfg.onset, "offset": cfg.offset, "min_on": int(min_on),
                    "min_off": int(min_off), "pad_on": int(pad_on), "pad_off": int(pad_off), "lag": lag, "max_events": max_events,
                    "events": torch.zeros((B, max_events, 2), dtype=torch.int32, device=self.device),
                    "ev_counts": torch.zeros(B, dtype=torch.int32, device=self.device),
                    "active": torch.zeros(B, dtype=torch.uint8, device=self.device),
                    "labels": torch.zeros((B, ld_in + lag), dtype=torch.uint8, device=self.device),
                    "lab_counts": torch.zeros(B, dtype=torch.int32, device=self.device)}

    def _endpoint_hyst_enqueue(self, ep, probs_ptr, counts_ptr, flags_ptr):
        return self._endpoint_enqueue(ep, probs_ptr, counts_ptr, flags_ptr, self.lib.uvad_endpoint_hyst_step)

    def endpoint_hyst_step(self, ep, probs: "torch.Tensor", counts: "torch.Tensor", start=None, end=None):
        """endpoint_step for a hysteresis endpointer: the same arguments and returns; active is 0 idle, 1 inside a confirmed interval,
        2 inside a candidate that has not reached min_on frames yet."""
        return self._endpoint_run(ep, self._endpoint_hyst_enqueue, probs, counts, start, end)

    # ------------------------------------------------------------------ live speech gate (uvad_gate_*)
    @staticmethod
    def _gate_cfg(dtype, cuts_cfg):
        """What gate_open and gate_group_open make of dtype and **cuts_cfg -> (the parameters with their defaults, the CutsCfg, the unit size)."""
        if dtype not in (torch.float32, torch.int16):
            raise ValueError(f"dtype must be torch.float32 or torch.int16, got {dtype}")
        q = dict(pad=0, max_len=0, min_len=0, hop=160, lead=0, tail=240)
        extra = set(cuts_cfg) - set(q)
        if extra:
            raise ValueError(f"unknown gate parameters {sorted(extra)} (pad, max_len, hop, lead, tail)")
        q.update(cuts_cfg)
        cfg = _lib.CutsCfg(*(int(q[k]) for k in ("pad", "max_len", "min_len", "hop", "lead", "tail")))
        return q, cfg, 2 if dtype == torch.int16 else 4

    def _gate_pair(self, x, n, what, ld, rows):
        """A gate step's (bytes, counts) input pair: x (rows, ld) uint8 (ld None: any width) and n (rows,) int32 on the GPU, or None, None
        where there is nothing to pass (ld None or 0) -> (x, n, columns of x), contiguous."""
        if x is None and n is None and not ld:
            return None, None, 0
        if not torch.is_tensor(x) or x.device != self.device or x.dtype != torch.uint8 or x.dim() != 2 or x.shape[0] != rows or \
                (ld is not None and x.shape[1] != ld):
            raise ValueError(f"{what} must be a ({rows}, {ld if ld is not None else 'ld'}) uint8 tensor on {self.device}")
        if not torch.is_tensor(n) or n.device != self.device or n.dtype != torch.int32 or tuple(n.shape) != (rows,):
            raise ValueError(f"{what}' counts must be an int32 tensor of shape ({rows},) on {self.device}")
        x, n = x.contiguous(), n.contiguous()
        return x, n, x.shape[1]

    def gate_open(self, B: int, chunk: int, ld_lab: int, dtype, lag_frames: int, history=None, ld_out=None, max_seg=None, **cuts_cfg):
        """Allocate and reset a speech gate of B slots (uvad_gate_reset): the streaming cuts_table + cuts_gather.  Every step takes a
        (B, chunk) block of samples of `dtype` (torch.int16 or torch.float32) and up to ld_lab finalised labels per slot and emits each
        slot's speech audio as fragments with records.  **cuts_cfg: pad, max_len, hop, lead, tail as cuts_open (min_len must be 0).
        lag_frames: how far the label frontier may trail floor(samples / hop) after a step; it sizes the history ring
        (uvad_gate_history) unless `history` samples are given.  ld_out / max_seg default to uvad_gate_max_out / uvad_gate_max_seg, which
        never truncate."""
        q, cfg, unit = self._gate_cfg(dtype, cuts_cfg)
        if history is None:
            history = int(self.lib.uvad_gate_history(C.byref(cfg), int(lag_frames), int(chunk)))
        history = int(history)
        with torch.cuda.device(self.device):
            nbytes = int(self.lib.uvad_gate_state_bytes(self.ctx, B, C.byref(cfg), unit, history)) if history >= 1 else 0
            auto_out = int(self.lib.uvad_gate_max_out(C.byref(cfg), int(ld_lab), int(chunk), history))
            auto_seg = int(self.lib.uvad_gate_max_seg(C.byref(cfg), int(ld_lab)))
            if nbytes == 0 or auto_out < 0 or auto_seg < 0:
                raise ValueError(f"bad gate configuration: B {B} (>= 1), chunk {chunk} (1 .. 2^24), ld_lab {ld_lab} (>= 0), lag_frames "
                                 f"{lag_frames} (>= 0), history {history} (chunk .. 2^31 - 1), pad {q['pad']} (0 .. 2^20), max_len {q['max_len']} "
                                 f"(0 .. 2^24), min_len {q['min_len']} (0), hop {q['hop']} (>= 1), lead {q['lead']} and tail {q['tail']} (>= 0)")
            ld_out = auto_out if ld_out is None else int(ld_out)
            max_seg = auto_seg if max_seg is None else int(max_seg)
            if ld_out < 0 or max_seg < 0:
                raise ValueError("ld_out and max_seg must be >= 0")
            state = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            self._check(self.lib.uvad_gate_reset(self.ctx, state.data_ptr(), nbytes, B, C.byref(cfg), unit, history, self._stream()))
            return {"state": state, "B": B, "chunk": int(chunk), "ld_lab": int(ld_lab), "dtype": dtype, "cfg": cfg, "history": history,
                    "lag_frames": int(lag_frames), "ld_out": ld_out, "max_seg": max_seg,
                    "out": torch.zeros((B, max(ld_out, 1)), dtype=dtype, device=self.device),
                    "seg": torch.zeros((B, max(max_seg, 1), 8), dtype=torch.int32, device=self.device),
                    "seg_counts": torch.zeros(B, dtype=torch.int32, device=self.device)}

    def _gate_enqueue(self, g, chunk_ptr, labels_ptr, lab_counts_ptr, flags_ptr):
        return self.lib.uvad_gate_step(self.ctx, chunk_ptr, g["chunk"], labels_ptr, g["ld_lab"], lab_counts_ptr, flags_ptr, g["B"],
                                       g["state"].data_ptr(), g["state"].numel(), g["out"].data_ptr() if g["ld_out"] else None, g["ld_out"],
                                       g["seg"].data_ptr() if g["max_seg"] else None, g["max_seg"], g["seg_counts"].data_ptr(), self._stream())

    def gate_step(self, g, chunk: "torch.Tensor", labels, lab_counts, start=None, end=None):
        """chunk (B, chunk) of the gate's dtype, labels (B, ld_lab) uint8 and lab_counts (B,) int32 on the GPU (None, None with ld_lab = 0);
        start / end as window_slots_step.  -> (out (B, ld_out), seg (B, max_seg, 8) int32 -- uvad_gate_seg rows {index, flags, first_frame,
        n_frames, offset lo / hi, n, n_stored} --, seg_counts (B,) int32), on the device and overwritten by the next step."""
        with torch.cuda.device(self.device):
            if not torch.is_tensor(chunk) or chunk.device != self.device or chunk.dtype != g["dtype"] or tuple(chunk.shape) != (g["B"], g["chunk"]):
                raise ValueError(f"chunk must be a ({g['B']}, {g['chunk']}) {g['dtype']} tensor on {self.device}")
            chunk = chunk.contiguous()
            lp = cp = None
            if g["ld_lab"]:                                                    # with ld_lab = 0 whatever is passed is not looked at
                labels, lab_counts, _ = self._gate_pair(labels, lab_counts, "labels", g["ld_lab"], g["B"])
                lp, cp = labels.data_ptr(), lab_counts.data_ptr()
            flags = self._slot_flags(g["B"], start, end)
            self._check(self._gate_enqueue(g, chunk.data_ptr(), lp, cp, flags.data_ptr() if flags is not None else None))
            return g["out"], g["seg"], g["seg_counts"]

    def gate_collect(self, g):
        """The records of the last step on the host -> [(slot, index, flags, first_frame, n_frames, fragment)]: fragment is a view of the
        n_stored samples in g["out"] (on the device, overwritten by the next step).  One synchronising copy of the records and counts."""
        with torch.cuda.device(self.device):
            counts = g["seg_counts"].cpu().numpy()
            seg = g["seg"].cpu().numpy()
        out = []
        for b in range(g["B"]):
            off = 0
            for r in seg[b, :min(int(counts[b]), g["max_seg"])]:
                ns = int(r[7])
                out.append((b, int(r[0]), int(r[1]), int(r[2]), int(r[3]), g["out"][b, off:off + ns]))
                off += ns
        return out

    # ------------------------------------------------------------------ live speech gate for fused groups (uvad_gate_group_*)
    def gate_group_open(self, fuse_state, chunk: int, ld_lab: int, dtype, lag_frames: int, decide_frames: int, history=None, best_history=None,
                        ld_out=None, max_seg=None, **cuts_cfg):
        """Allocate and reset a group gate over the G groups of `fuse_state` (fuse_open's): the streaming cuts_table + fuse_pick +
        cuts_gather.  Every step takes the (B, chunk) block of samples of `dtype` the group members' rows sit in, the step's best bytes and
        up to ld_lab finalised labels per group, and emits each group's speech audio, each cut whole from the member that won most of its
        first `decide_frames` frames.  **cuts_cfg, lag_frames as gate_open; history / best_history default to uvad_gate_group_history /
        uvad_gate_group_best_history, ld_out / max_seg to uvad_gate_group_max_out / uvad_gate_max_seg, which never truncate."""
        q, cfg, unit = self._gate_cfg(dtype, cuts_cfg)
        chunk, ld_lab, lag_frames, D = int(chunk), int(ld_lab), int(lag_frames), int(decide_frames)
        if history is None:
            history = self.lib.uvad_gate_group_history(C.byref(cfg), lag_frames, chunk, D)
        if best_history is None:
            best_history = self.lib.uvad_gate_group_best_history(C.byref(cfg), lag_frames, chunk, D)
        history, best_history = int(history), int(best_history)
        with torch.cuda.device(self.device):
            self._fuse_configure(fuse_state)
            ok = 1 <= history < 2 ** 31 and 1 <= best_history < 2 ** 31
            nbytes = int(self.lib.uvad_gate_group_state_bytes(self.ctx, C.byref(cfg), unit, history, best_history)) if ok else 0
            auto_out = int(self.lib.uvad_gate_group_max_out(C.byref(cfg), ld_lab, chunk, D))
            auto_seg = int(self.lib.uvad_gate_max_seg(C.byref(cfg), ld_lab))
            if nbytes == 0 or auto_out < 0 or auto_seg < 0 or history < chunk:
                raise ValueError(f"bad group gate configuration: chunk {chunk} (1 .. 2^24), ld_lab {ld_lab} (>= 0), lag_frames {lag_frames} (>= 0), "
                                 f"decide_frames {D} (1 .. 2^24), history {history} (chunk .. 2^31 - 1), best_history {best_history} (1 .. 2^31 - 1), "
                                 f"pad {q['pad']} (0 .. 2^20), max_len {q['max_len']} (0 .. 2^24), min_len {q['min_len']} (0), hop {q['hop']} (>= 1), "
                                 f"lead {q['lead']} and tail {q['tail']} (>= 0)")
            ld_out = auto_out if ld_out is None else int(ld_out)
            max_seg = auto_seg if max_seg is None else int(max_seg)
            if ld_out < 0 or max_seg < 0:
                raise ValueError("ld_out and max_seg must be >= 0")
            G = fuse_state["G"]
            state = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            self._check(self.lib.uvad_gate_group_reset(self.ctx, state.data_ptr(), nbytes, C.byref(cfg), unit, history, best_history, D,
                                                       self._stream()))
            return {"state": state, "fuse": fuse_state, "G": G, "B": int(fuse_state["members"].max()) + 1, "chunk": chunk, "ld_lab": ld_lab,
                    "dtype": dtype, "cfg": cfg, "history": history, "best_history": best_history, "decide_frames": D, "lag_frames": lag_frames,
                    "ld_out": ld_out, "max_seg": max_seg,
                    "out": torch.zeros((G, max(ld_out, 1)), dtype=dtype, device=self.device),
                    "seg": torch.zeros((G, max(max_seg, 1), 8), dtype=torch.int32, device=self.device),
                    "seg_counts": torch.zeros(G, dtype=torch.int32, device=self.device)}

    def _gate_group_enqueue(self, g, chunk_ptr, B, best_ptr, ld_best, best_counts_ptr, labels_ptr, lab_counts_ptr, gflags_ptr, rflags_ptr):
        return self.lib.uvad_gate_group_step(self.ctx, chunk_ptr, g["chunk"], B, best_ptr, ld_best, best_counts_ptr, labels_ptr, g["ld_lab"],
                                             lab_counts_ptr, gflags_ptr, rflags_ptr, g["state"].data_ptr(), g["state"].numel(),
                                             g["out"].data_ptr() if g["ld_out"] else None, g["ld_out"],
                                             g["seg"].data_ptr() if g["max_seg"] else None, g["max_seg"], g["seg_counts"].data_ptr(), self._stream())

    def gate_group_step(self, g, chunk: "torch.Tensor", best, best_counts, labels, lab_counts, start=None, end=None, row_flags=None):
        """chunk (B, chunk) of the gate's dtype, B above the largest member row; best (G, ld_best) uint8 and best_counts (G,) int32: the
        step's fuse best bytes and group lengths (None, None: none); labels (G, ld_lab) uint8 and lab_counts (G,) int32 (None, None with
        ld_lab = 0); start / end: the GROUPS whose session starts with / ends after this step, as window_slots_step's; row_flags (B,) uint8
        on the GPU: the rows' flag bytes for the lockstep check, or None.  -> (out (G, ld_out), seg (G, max_seg, 8) int32 -- uvad_gate_seg
        rows, the member position in bits 8 .. 15 of flags --, seg_counts (G,) int32), on the device and overwritten by the next step."""
        G = g["G"]
        with torch.cuda.device(self.device):
            if not torch.is_tensor(chunk) or chunk.device != self.device or chunk.dtype != g["dtype"] or chunk.dim() != 2 or \
                    chunk.shape[1] != g["chunk"] or chunk.shape[0] < g["B"]:
                raise ValueError(f"chunk must be a (>= {g['B']}, {g['chunk']}) {g['dtype']} tensor on {self.device}")
            chunk = chunk.contiguous()
            best, best_counts, ld_best = self._gate_pair(best, best_counts, "best", None, G)
            labels, lab_counts, _ = self._gate_pair(labels, lab_counts, "labels", g["ld_lab"], G)
            if row_flags is not None and (not torch.is_tensor(row_flags) or row_flags.device != self.device or row_flags.dtype != torch.uint8 or
                                          tuple(row_flags.shape) != (chunk.shape[0],)):
                raise ValueError(f"row_flags must be a ({chunk.shape[0]},) uint8 tensor on {self.device}")
            flags = self._slot_flags(G, start, end)
            self._fuse_configure(g["fuse"])
            ptr = lambda t: t.data_ptr() if t is not None else None
            self._check(self._gate_group_enqueue(g, chunk.data_ptr(), chunk.shape[0], ptr(best), ld_best, ptr(best_counts), ptr(labels),
                                                 ptr(lab_counts), ptr(flags), ptr(row_flags)))
            return g["out"], g["seg"], g["seg_counts"]

    def gate_group_collect(self, g):
        """The records of the last step on the host -> per group a list of dicts {"index", "flags", "first_frame", "n_frames", "offset", "n",
        "channel" (the member position), "row" (its input row), "fragment" (a view of the n_stored samples in g["out"], on the device,
        overwritten by the next step)}.  One synchronising copy of the records and counts."""
        with torch.cuda.device(self.device):
            counts = g["seg_counts"].cpu().numpy()
            seg = g["seg"].cpu().numpy()
        groups = g["fuse"]["groups"]
        out = []
        for b in range(g["G"]):
            off, recs = 0, []
            for r in seg[b, :min(int(counts[b]), g["max_seg"])]:
                ns, ch = int(r[7]), (int(r[1]) >> 8) & 0xff
                recs.append({"index": int(r[0]), "flags": int(r[1]) & 0xff, "first_frame": int(r[2]), "n_frames": int(r[3]),
                             "offset": int(r[4]) & 0xffffffff | int(r[5]) << 32, "n": int(r[6]), "channel": ch, "row": int(groups[b][ch]),
                             "fragment": g["out"][b, off:off + ns]})
                off += ns
            out.append(recs)
        return out

    # ------------------------------------------------------------------ what the three training families share
    # A handle carries its family, h["family"]: the library's entries are uvad_<family>_train_*; the record holds the packed key list of a
    # handle and the words of the family's scalar record.
    _TRAIN_FAMILIES = {"head": (lambda rt, h: rt.head_train_keys(), _lib.HEAD_TRAIN_SCALAR_WORDS),
                       "lstm": (lambda rt, h: rt.lstm_train_keys(h["layers"]), _lib.LSTM_TRAIN_SCALAR_WORDS),
                       "sincnet": (lambda rt, h: rt.sincnet_train_keys(h["first_stage"]), _lib.HEAD_TRAIN_SCALAR_WORDS)}
    _TRAIN_BLOCKS = (("weights", _lib.HEAD_TRAIN_MASTERS), ("grad", _lib.HEAD_TRAIN_GRAD), ("m", _lib.HEAD_TRAIN_M), ("v", _lib.HEAD_TRAIN_V))

    def _train_fn(self, h, op: str):
        return getattr(self.lib, f"uvad_{h['family']}_train_{op}")

    def _train_configure(self, h):
        """The handle's configuration (an LSTM handle: its dropout setting too) on the context, before every call on the handle: host
        only, the context serves any number of handles."""
        self._check(self._train_fn(h, "configure")(self.ctx, C.byref(h["cfg"])))
        if h["family"] == "lstm":
            self._check(self.lib.uvad_lstm_train_set_dropout(self.ctx, h.get("dropout", 0.0), h.get("seed", 0)))

    _lstm_train_configure = _train_configure   # the name the LSTM training tests call it by

    def _train_apply(self, h):
        with torch.cuda.device(self.device):
            self._train_configure(h)
            self._check(self._train_fn(h, "apply")(self.ctx, h["state"].data_ptr(), h["state"].numel(), self._stream()))

    def _train_block(self, h, which: int) -> np.ndarray:
        self._check(self._train_fn(h, "read")(self.ctx, h["state"].data_ptr(), h["state"].numel(), which, h["out"].data_ptr(), self._stream()))
        return h["out"].cpu().numpy().copy()

    def _train_read(self, h):
        """Copy the state to the host (synchronises) -> ({"weights", "grad", "m", "v": {torch key: tensor}, "scalars" (the raw record: what
        the family's _write takes back), "frames", "step", "bias_correction1", "bias_correction2" (1 - beta^step)}, the record's words);
        the family adds what else its record or state holds."""
        keys, words = self._TRAIN_FAMILIES[h["family"]]
        with torch.cuda.device(self.device):
            self._train_configure(h)
            out = {}
            for name, which in self._TRAIN_BLOCKS:
                flat, off, d = self._train_block(h, which), 0, {}
                for key, shape in keys(self, h):
                    cnt = int(np.prod(shape))
                    d[key] = torch.from_numpy(flat[off:off + cnt].reshape(shape).copy())
                    off += cnt
                out[name] = d
            w = self._train_block(h, _lib.HEAD_TRAIN_SCALARS)[:words]
        out["scalars"] = torch.from_numpy(w.view(np.int32).copy())
        out["frames"] = int(w[2:4].view(np.uint64)[0])
        out["step"] = int(w[4:6].view(np.uint64)[0])
        out["bias_correction1"], out["bias_correction2"] = float(w[6]), float(w[7])
        return out, w

    def _train_commit(self, h):
        with torch.cuda.device(self.device):
            self._train_configure(h)
            self._check(self._train_fn(h, "commit")(self.ctx, h["state"].data_ptr(), h["state"].numel()))
            self._weights_gen = getattr(self, "_weights_gen", 0) + 1

    # ------------------------------------------------------------------ head fine-tuning (uvad_head_train_*)
    def head_train_keys(self):
        """[(torch key, shape)] of the trainable tensors in the packed order of uvad_head_train_read (state_dict order)."""
        m = self._mc_c
        k = m.hidden * (2 if m.bidirectional else 1)
        out = []
        for l in range(m.lin_layers):
            out += [(f"linear.{l}.weight", (m.lin_hidden, k)), (f"linear.{l}.bias", (m.lin_hidden,))]
            k = m.lin_hidden
        return out + [("classifier.weight", (1, k)), ("classifier.bias", (1,))]

    def head_train_open(self, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, segment: int = 0):
        """Allocate and reset a fine-tuning state for the head (uvad_head_train_reset): f32 master copies of linear.* / classifier.* as
        finalized, Adam moments, the gradient accumulator.  The LSTM stack stays frozen.  segment: frames per gradient partial (0 = the
        library's default).  The handle owns the state and the workspace."""
        cfg = _lib.HeadTrainCfg(float(lr), float(betas[0]), float(betas[1]), float(eps), int(segment))
        with torch.cuda.device(self.device):
            self._check(self.lib.uvad_head_train_configure(self.ctx, C.byref(cfg)))
            P = int(self.lib.uvad_head_train_param_count(self.ctx))
            h = {"family": "head", "cfg": cfg, "P": P, "state": torch.empty(int(self.lib.uvad_head_train_state_bytes(self.ctx)), dtype=torch.uint8, device=self.device),
                 "ws": None, "out": torch.zeros(max(P, _lib.HEAD_TRAIN_SCALAR_WORDS), dtype=torch.float32, device=self.device)}
            self._check(self.lib.uvad_head_train_reset(self.ctx, h["state"].data_ptr(), h["state"].numel(), self._stream()))
            return h

    def head_train_grad(self, h, x: "torch.Tensor", labels=None, lengths=None, weights=None, dz=None, want_probs: bool = False,
                        want_grad_x: bool = False):
        """One micro-batch (uvad_head_train_grad): x (B, T, hidden x directions) f32 LSTM output on the GPU (taps(lin=False)[0], which may be
        cached), labels (B, T) uint8, lengths (B,) valid frames per row, weights (B, T) f32 frame weights, or dz (B, T) f32 in place of
        the loss gradient (labels and weights are then not read).  Adds the gradients, the loss sum and the frame count into the state;
        no copy to the host and no synchronisation, so once the workspace has the batch shape's size the call can be captured.
        -> (probs (B, T) | None, grad_x (B, T, D0) | None); head_train_batch_loss gives the call's mean loss."""
        with torch.cuda.device(self.device):
            x = self._dev_f32(x, "x")
            B, T, D0 = x.shape
            if D0 != self._mc_c.hidden * (2 if self._mc_c.bidirectional else 1):
                raise ValueError(f"x has {D0} columns, the LSTM output has {self._mc_c.hidden * (2 if self._mc_c.bidirectional else 1)}")
            if dz is None and labels is None:
                raise ValueError("labels or dz must be given")
            ptr = lambda t: (t.data_ptr(), t.stride(0)) if t is not None else (None, 0)
            for t, dt, name in ((labels, torch.uint8, "labels"), (weights, torch.float32, "weights"), (dz, torch.float32, "dz")):
                if t is not None:
                    if not torch.is_tensor(t) or t.device != self.device or tuple(t.shape) != (B, T):
                        raise ValueError(f"{name} must be a ({B}, {T}) tensor on {self.device}")
                    self._rows_2d(t, dt, name)
            n = None if lengths is None else self._dev_lens(lengths, B, T, torch.int32, "lengths (frames)")
            self._train_configure(h)
            need = int(self.lib.uvad_head_train_ws_bytes(self.ctx, B, T))
            if h["ws"] is None or h["ws"].numel() < need:
                h["ws"] = torch.zeros(need, dtype=torch.uint8, device=self.device)
            probs = torch.zeros((B, T), dtype=torch.float32, device=self.device) if want_probs else None
            grad_x = torch.empty((B, T, D0), dtype=torch.float32, device=self.device) if want_grad_x else None
            self._check(self.lib.uvad_head_train_grad(self.ctx, x.data_ptr(), B, T, n.data_ptr() if n is not None else None,
                                                      *ptr(labels), *ptr(weights), *ptr(dz), *ptr(probs),
                                                      grad_x.data_ptr() if grad_x is not None else None,
                                                      h["state"].data_ptr(), h["state"].numel(), h["ws"].data_ptr(), h["ws"].numel(), self._stream()))
            h["_keep"] = (x, labels, weights, dz, n)   # the launches read them after this call returns
            return probs, grad_x

    def head_train_batch_loss(self, h) -> "torch.Tensor":
        """The most recent head_train_grad's mean loss over its valid frames, a 0-d f64 tensor on the device (no synchronisation)."""
        head = h["ws"][:16]
        return head[:8].view(torch.float64)[0] / head[8:].view(torch.int64)[0].to(torch.float64)

    def head_train_apply(self, h):
        """One Adam step from the accumulated gradients divided by the accumulated frame count (uvad_head_train_apply)."""
        self._train_apply(h)

    def head_train_read(self, h) -> dict:
        """Copy the state to the host (synchronises) -> {"weights", "grad", "m", "v": {torch key: tensor}, "loss" (accumulated sum),
        "frames", "step", "bias_correction1", "bias_correction2" (1 - beta^step), "scalars" (the raw record)}."""
        out, w = self._train_read(h)
        out["loss"] = float(w[0:2].view(np.float64)[0])
        return out

    def head_train_state_dict(self, h) -> dict:
        """The adapted head tensors keyed by torch key, ready to merge into a checkpoint (synchronises)."""
        return self.head_train_read(h)["weights"]

    def head_train_commit(self, h):
        """Make this runtime serve the adapted head (uvad_head_train_commit: synchronises, re-finalizes).  Graphs captured before are
        stale, as after load_state_dict."""
        self._train_commit(h)

    # ------------------------------------------------------------------ LSTM training (uvad_lstm_train_*)
    def _lstm_train_shape(self, first_layer: int):
        m = self._mc_c
        dirs = 2 if m.bidirectional else 1
        return (m.in_dim if first_layer == 0 else m.hidden * dirs), m.hidden, dirs, m.num_layers, first_layer

    def lstm_train_keys(self, layers: int = 1):
        """[(torch key, shape)] of the trainable tensors of the top `layers` LSTM layers in the packed order of uvad_lstm_train_read
        (state_dict order: per layer, forward then _reverse, weight_ih, weight_hh, bias_ih, bias_hh)."""
        Din, H, dirs, L, first = self._lstm_train_shape(self._mc_c.num_layers - int(layers))
        out = []
        for k in range(first, L):
            K = Din if k == first else H * dirs
            for d in range(dirs):
                suf = f"_l{k}" + ("_reverse" if d else "")
                out += [(f"lstm.weight_ih{suf}", (4 * H, K)), (f"lstm.weight_hh{suf}", (4 * H, H)), (f"lstm.bias_ih{suf}", (4 * H,)),
                        (f"lstm.bias_hh{suf}", (4 * H,))]
        return out

    def lstm_train_open(self, layers: int = 1, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, segment: int = 0,
                        dropout: float = 0.0, seed: int = 0):
        """Allocate and reset a training state for the top `layers` layers of the LSTM stack (uvad_lstm_train_reset): f32 master copies of
        their tensors as loaded, Adam moments, the gradient accumulator; first_layer = num_layers - layers, the layers below stay frozen.
        dropout, seed: nn.LSTM's dropout between the learning layers (uvad_lstm_train_set_dropout; 0 = none, the kernels of a run without
        it).  The handle owns the state and the workspace."""
        dropout = float(dropout)
        if not 0.0 <= dropout < 1.0:
            raise ValueError("dropout must lie in [0, 1)")
        layers = int(layers)
        if not 1 <= layers <= self._mc_c.num_layers:
            raise ValueError(f"layers must lie in 1 .. {self._mc_c.num_layers}")
        cfg = _lib.LstmTrainCfg(float(lr), float(betas[0]), float(betas[1]), float(eps), int(segment), self._mc_c.num_layers - layers)
        with torch.cuda.device(self.device):
            self._check(self.lib.uvad_lstm_train_configure(self.ctx, C.byref(cfg)))
            self._check(self.lib.uvad_lstm_train_set_dropout(self.ctx, dropout, int(seed) & 0xFFFFFFFFFFFFFFFF))
            P = int(self.lib.uvad_lstm_train_param_count(self.ctx))
            h = {"family": "lstm", "cfg": cfg, "P": P, "layers": layers, "first_layer": cfg.first_layer, "ws": None, "bt": None,
                 "dropout": dropout, "seed": int(seed) & 0xFFFFFFFFFFFFFFFF,
                 "state": torch.empty(int(self.lib.uvad_lstm_train_state_bytes(self.ctx)), dtype=torch.uint8, device=self.device),
                 "out": torch.zeros(max(P, _lib.LSTM_TRAIN_SCALAR_WORDS), dtype=torch.float32, device=self.device)}
            self._check(self.lib.uvad_lstm_train_reset(self.ctx, h["state"].data_ptr(), h["state"].numel(), self._stream()))
            return h

    def lstm_train_input(self, x: "torch.Tensor", lengths=None, layers: int = 1) -> "torch.Tensor":
        """The input of layer first_layer = num_layers - layers for the features x (B, T, encoding_dim): the frozen prefix's output, which a
        caller caches across epochs.  x itself when every layer learns; otherwise the LSTM tap of a sibling context holding a
        first_layer-layer copy of the model as loaded (classify + taps).  Host code only."""
        first = self._mc_c.num_layers - int(layers)
        if first == 0:
            return self._dev_f32(x, "x")
        sib = self._lstm_prefix.get(first)
        if sib is None:
            top = re.compile(r"(?:^|\.)lstm\.(?:(\d+)\.)?\w+_l(\d+)(?:_reverse)?$")

            def frozen(key):
                m = top.search(key)
                return m is None or int(m.group(1) if m.group(1) is not None else m.group(2)) < first
            rt = VadRuntime(self.device, model=dict(self.model_cfg, lstm=dict(self.model_cfg["lstm"], num_layers=first)))
            rt.load_state_dict({k: v for k, v in self._loaded_sd.items() if frozen(k) and ".sincnet." not in k and not k.startswith("sincnet.")})
            sib = self._lstm_prefix[first] = rt
        sib.classify(x, want_logits=True, want_probs=False, lengths=lengths)
        return sib.taps(lin=False)[0]

    def lstm_train_draws(self, h) -> int:
        """How many dropout masks the handle's forward calls have drawn: the 64-bit count at byte 56 of the state (synchronises)."""
        return int(h["state"][56:64].cpu().numpy().view(np.uint64)[0])

    def dropout_apply(self, x: "torch.Tensor", layer: int, draw: int, p: float, seed: int, out=None) -> "torch.Tensor":
        """The mask of uvad_lstm_train_set_dropout as a stand-alone pass (uvad_dropout_apply): x (..., cols) f32 on the GPU, rows = every
        leading dimension flattened (the mask's frame index), cols a multiple of 4 up to 2048 -> keep ? x / (1 - p) : +0.  out: a tensor of
        x's shape to write (x itself: in place); None allocates one.  For input dropout on cached features."""
        with torch.cuda.device(self.device):
            x = self._dev_f32(x, "x")
            if out is None:
                out = torch.empty_like(x)
            if not (torch.is_tensor(out) and out.device == x.device and out.dtype == torch.float32 and out.shape == x.shape and out.is_contiguous()):
                raise ValueError("out must be a contiguous f32 tensor of x's shape on x's device")
            self._check(self.lib.uvad_dropout_apply(x.data_ptr(), out.data_ptr(), x.numel() // x.shape[-1], x.shape[-1], int(layer),
                                                    int(draw) & 0xFFFFFFFFFFFFFFFF, float(p), int(seed) & 0xFFFFFFFFFFFFFFFF, self._stream()))
            return out

    # ------------------------------------------------------------------ noise mixing of training batches (uvad_mix_*)
    @staticmethod
    def mix_amp_table(snr, snr_steps: int) -> np.ndarray:
        """The noise-to-speech amplitude ratios of snr_steps SNR steps over snr = (lo, hi) dB (a number: that one SNR)."""
        lo, hi = (float(snr), float(snr)) if np.isscalar(snr) else (float(snr[0]), float(snr[1]))
        Q = int(snr_steps)
        if Q < 1:
            raise ValueError("snr_steps must be at least 1")
        return np.array([10 ** (-(lo + (hi - lo) * (q + 0.5) / Q) / 20) for q in range(Q)], np.float64)

    def mix_open(self, bank, clip_lengths, snr=(10, 20), mix_prob: float = 0.5, snr_steps: int = 1024, max_seg: int = 8, seed: int = 0):
        """Allocate and reset a noise-mix state (uvad_mix_reset).  bank: the noise clips back to back, a 1-D f32 tensor (moved to this
        device; the handle keeps it alive), clip_lengths: samples per clip.  snr (lo, hi) dB, mix_prob, max_seg and seed as
        include/uvad.h; the amplitude table is mix_amp_table(snr, snr_steps).  The clip energies are computed on the device here."""
        lens = [int(v) for v in clip_lengths]
        if not lens or min(lens) < 1:
            raise ValueError("every noise clip needs at least 1 sample")
        if not 0.0 <= float(mix_prob) <= 1.0:
            raise ValueError("mix_prob must lie in [0, 1]")
        if not 1 <= int(max_seg) <= _lib.MIX_MAX_SEG:
            raise ValueError(f"max_seg must lie in [1, {_lib.MIX_MAX_SEG}]")
        first = np.zeros(len(lens) + 1, np.int64)
        first[1:] = np.cumsum(lens)
        amp = self.mix_amp_table(snr, snr_steps)
        with torch.cuda.device(self.device):
            bank = torch.as_tensor(bank, dtype=torch.float32).reshape(-1).to(self.device).contiguous()
            if bank.numel() != int(first[-1]):
                raise ValueError(f"bank holds {bank.numel()} samples, the clip lengths add up to {int(first[-1])}")
            cfg = _lib.MixCfg(float(mix_prob), len(amp), amp.ctypes.data_as(C.POINTER(C.c_double)), int(max_seg), int(seed) & 0xFFFFFFFFFFFFFFFF)
            st = {"cfg": cfg, "amp": amp, "bank": bank, "first": first, "n_clips": len(lens), "max_seg": int(max_seg),
                  "plan_words": _lib.MIX_PLAN_HEAD + _lib.MIX_SEG_WORDS * int(max_seg), "ws": None,
                  "state": torch.zeros(int(self.lib.uvad_mix_state_bytes(C.byref(cfg), len(lens))), dtype=torch.uint8, device=self.device)}
            self._check(self.lib.uvad_mix_reset(self.ctx, st["state"].data_ptr(), st["state"].numel(), C.byref(cfg), bank.data_ptr(),
                                                first.ctypes.data_as(C.POINTER(C.c_int64)), len(lens), self._stream()))
            return st

    def mix_draws(self, st) -> int:
        """How many steps the state has drawn: the 64-bit count at byte 56 (synchronises)."""
        return int(st["state"][56:64].cpu().numpy().view(np.uint64)[0])

    def mix_clip_energies(self, st) -> np.ndarray:
        """The clips' energies as uvad_mix_reset computed them (synchronises)."""
        off = 256 + (8 * (st["n_clips"] + 1) + 255) // 256 * 256
        return st["state"][off:off + 8 * st["n_clips"]].cpu().numpy().view(np.float64).copy()

    def mix_row_energies(self, st, B: int) -> np.ndarray:
        """The row energies of the state's last step (synchronises)."""
        return st["ws"][256:256 + 8 * B].cpu().numpy().view(np.float64).copy()

    def _augment_args(self, st, pcm, nsamp, out, plan, ws_bytes):
        """What uvad_mix_step / uvad_reverb_step (and their _apply forms) share: the checked batch, the output and plan tensors, the
        state's workspace grown to ws_bytes(B), and the argument lists in front of and behind (row0, draw).  -> (head, tail, out, plan)"""
        i16 = pcm.dtype == torch.int16
        if i16:
            if pcm.device != self.device:
                raise RuntimeError(f"pcm must be on {self.device}")
            pcm = pcm.contiguous()
        else:
            pcm = self._dev_f32(pcm, "pcm")
        B, S = pcm.shape
        if out is None:
            out = torch.empty((B, S), dtype=torch.float32, device=self.device)
        if not (torch.is_tensor(out) and out.device == self.device and out.dtype == torch.float32 and tuple(out.shape) == (B, S) and
                out.is_contiguous()):
            raise ValueError("out must be a contiguous f32 tensor of pcm's shape on pcm's device")
        if plan is True:
            plan = torch.zeros((B, st["plan_words"]), dtype=torch.int32, device=self.device)
        elif plan is False:
            plan = None
        elif not (torch.is_tensor(plan) and plan.device == self.device and plan.dtype == torch.int32 and
                  tuple(plan.shape) == (B, st["plan_words"]) and plan.is_contiguous()):
            raise ValueError(f"plan must be a contiguous int32 tensor of shape ({B}, {st['plan_words']}) on pcm's device")
        n = None if nsamp is None else self._dev_lens(nsamp, B, S, torch.int64, "nsamp (samples)")
        need = int(ws_bytes(B))
        if st["ws"] is None or st["ws"].numel() < need:
            st["ws"] = torch.zeros(need, dtype=torch.uint8, device=self.device)
        head = (self.ctx, pcm.data_ptr(), _lib.INGEST_I16 if i16 else _lib.INGEST_F32, B, S, None if n is None else n.data_ptr(),
                out.data_ptr(), None if plan is None else plan.data_ptr())
        tail = (st["state"].data_ptr(), st["state"].numel(), st["ws"].data_ptr(), st["ws"].numel(), self._stream())
        return head, tail, out, plan

    def mix_step(self, st, pcm: "torch.Tensor", nsamp=None, out=None, plan=False, draw=None, row0: int = 0):
        """pcm (B, S) f32 or int16 on the GPU -> the batch with noise mixed in, (B, S) f32 (uvad_mix_step: a fresh draw per call).
        nsamp: samples per row (B,), as fbank's lengths; out: the f32 tensor to write (pcm itself: in place; None allocates one);
        plan: True also returns the plan record (B, 4 + 4 max_seg) int32, or pass the tensor to write.  draw: an explicit draw ordinal
        (uvad_mix_apply: no state update), with row0 the index the first row draws under.  After the first call with a batch size
        nothing is allocated when out (and plan) are given: the call can be captured."""
        with torch.cuda.device(self.device):
            head, tail, out, plan = self._augment_args(st, pcm, nsamp, out, plan, lambda B: self.lib.uvad_mix_ws_bytes(B, st["max_seg"]))
            if draw is None:
                self._check(self.lib.uvad_mix_step(*head, *tail))
            else:
                self._check(self.lib.uvad_mix_apply(*head, int(row0), int(draw) & 0xFFFFFFFFFFFFFFFF, *tail))
            return out if plan is None else (out, plan)

    # ------------------------------------------------------------------ reverberation of training batches (uvad_reverb_*)
    def reverb_open(self, bank, rir_lengths, prob: float = 0.5, normalize: bool = True, align: bool = True, max_taps: int = 0, seed: int = 0):
        """Allocate and reset a reverberation state (uvad_reverb_reset).  bank: the room impulse responses back to back, a 1-D f32
        tensor (moved to this device; the handle keeps it alive), rir_lengths: taps per response.  prob, normalize, align, max_taps
        and seed as include/uvad.h.  The delays (direct paths) are computed on the device here."""
        lens = [int(v) for v in rir_lengths]
        if not lens or min(lens) < 1:
            raise ValueError("every impulse response needs at least 1 tap")
        if not 0.0 <= float(prob) <= 1.0:
            raise ValueError("prob must lie in [0, 1]")
        if int(max_taps) < 0:
            raise ValueError("max_taps must be >= 0")
        first = np.zeros(len(lens) + 1, np.int64)
        first[1:] = np.cumsum(lens)
        with torch.cuda.device(self.device):
            bank = torch.as_tensor(bank, dtype=torch.float32).reshape(-1).to(self.device).contiguous()
            if bank.numel() != int(first[-1]):
                raise ValueError(f"bank holds {bank.numel()} taps, the response lengths add up to {int(first[-1])}")
            cfg = _lib.ReverbCfg(float(prob), int(bool(normalize)), int(bool(align)), int(max_taps), int(seed) & 0xFFFFFFFFFFFFFFFF)
            st = {"cfg": cfg, "bank": bank, "first": first, "n_rirs": len(lens), "plan_words": _lib.REVERB_PLAN_WORDS, "ws": None,
                  "state": torch.zeros(int(self.lib.uvad_reverb_state_bytes(C.byref(cfg), len(lens))), dtype=torch.uint8, device=self.device)}
            self._check(self.lib.uvad_reverb_reset(self.ctx, st["state"].data_ptr(), st["state"].numel(), C.byref(cfg), bank.data_ptr(),
                                                   first.ctypes.data_as(C.POINTER(C.c_int64)), len(lens), self._stream()))
            return st

    def reverb_draws(self, st) -> int:
        """How many steps the state has drawn: the 64-bit count at byte 56 (synchronises)."""
        return int(st["state"][56:64].cpu().numpy().view(np.uint64)[0])

    def reverb_delays(self, st) -> np.ndarray:
        """The responses' delays (direct paths) as uvad_reverb_reset computed them (synchronises)."""
        pad = lambda v: (v + 255) // 256 * 256
        off = 256 + pad(8 * (st["n_rirs"] + 1)) + pad(4 * st["n_rirs"])
        return st["state"][off:off + 4 * st["n_rirs"]].cpu().numpy().view(np.int32).copy()

    def reverb_step(self, st, pcm: "torch.Tensor", nsamp=None, out=None, plan=False, draw=None, row0: int = 0):
        """pcm (B, S) f32 or int16 on the GPU -> the batch with the drawn rows reverberated, (B, S) f32 (uvad_reverb_step: a fresh draw
        per call).  nsamp: samples per row (B,), as fbank's lengths; out: the f32 tensor to write (never pcm itself; None allocates
        one); plan: True also returns the plan record (B, 4) int32, or pass the tensor to write.  draw: an explicit draw ordinal
        (uvad_reverb_apply: no state update), with row0 the index the first row draws under.  After the first call with a batch size
        nothing is allocated when out (and plan) are given: the call can be captured."""
        with torch.cuda.device(self.device):
            head, tail, out, plan = self._augment_args(st, pcm, nsamp, out, plan, self.lib.uvad_reverb_ws_bytes)
            if draw is None:
                self._check(self.lib.uvad_reverb_step(*head, *tail))
            else:
                self._check(self.lib.uvad_reverb_apply(*head, int(row0), int(draw) & 0xFFFFFFFFFFFFFFFF, *tail))
            return out if plan is None else (out, plan)

    # ------------------------------------------------------------------ training batches drawn on the device (uvad_sampler_*)
    def sampler_open(self, pcm, rec_lengths, supervisions, window: int, min_keep: int, geometry: str, half: int = 496, step: int = 270,
                     datasets=None, weights=None, shuffle: bool = True, drop_last: bool = False, pad: bool = False, seed: int = 0,
                     batch: int = 0):
        """Allocate and reset a sampler state (uvad_sampler_reset).  pcm: the recordings back to back, a 1-D f32 or int16 tensor (moved to
        this device; the handle keeps it alive); rec_lengths: samples per recording; supervisions: per recording, an (n, 2) table of
        {start, end} in samples of that recording.  window, min_keep in samples; geometry "fbank" or "sincnet" (half, step: the
        waveform grid's receptive-field half width and frame step); datasets: each recording's dataset index (None: one dataset),
        weights: one per dataset; shuffle, drop_last (with batch, the batch size it refers to), pad and seed as include/uvad.h."""
        lens = [int(v) for v in rec_lengths]
        if not lens or min(lens) < 1:
            raise ValueError("every recording needs at least 1 sample")
        if geometry not in ("fbank", "sincnet"):
            raise ValueError(f"unknown geometry {geometry!r} (fbank, sincnet)")
        if len(supervisions) != len(lens):
            raise ValueError(f"{len(supervisions)} supervision tables for {len(lens)} recordings")
        R = len(lens)
        first = np.zeros(R + 1, np.int64)
        first[1:] = np.cumsum(lens)
        tables = [np.asarray(s, np.int64).reshape(-1, 2) for s in supervisions]
        sup_first = np.zeros(R + 1, np.int32)
        sup_first[1:] = np.cumsum([len(t) for t in tables])
        sup = np.ascontiguousarray(np.concatenate(tables) if tables else np.zeros((0, 2)), np.int64)
        rec_set = np.zeros(R, np.int32) if datasets is None else np.ascontiguousarray(datasets, np.int32)
        if rec_set.shape != (R,):
            raise ValueError(f"datasets must name one dataset per recording ({R})")
        w = np.ones(int(rec_set.max()) + 1, np.float64) if weights is None else np.ascontiguousarray(weights, np.float64).reshape(-1)
        D = len(w)
        with torch.cuda.device(self.device):
            pcm = torch.as_tensor(pcm)
            if pcm.dtype != torch.int16:
                pcm = pcm.to(torch.float32)
            pcm = pcm.reshape(-1).to(self.device).contiguous()
            if pcm.numel() != int(first[-1]):
                raise ValueError(f"pcm holds {pcm.numel()} samples, the recording lengths add up to {int(first[-1])}")
            fmt = _lib.INGEST_I16 if pcm.dtype == torch.int16 else _lib.INGEST_F32
            cfg = _lib.SamplerCfg(int(window), int(min_keep), _lib.SAMPLER_FBANK if geometry == "fbank" else _lib.SAMPLER_SINCNET, int(half),
                                  int(step), int(bool(shuffle)), int(bool(drop_last)), int(bool(pad)), int(batch), int(seed) & 0xFFFFFFFFFFFFFFFF)
            frames = self.lib.uvad_num_frames if geometry == "fbank" else self.lib.uvad_sincnet_num_frames
            st = {"cfg": cfg, "pcm": pcm, "first": first, "R": R, "D": D, "W": int(window), "T": int(frames(self.ctx, int(window))), "ws": None,
                  "plan_words": _lib.SAMPLER_PLAN_WORDS, "bufs": {},
                  "state": torch.zeros(max(int(self.lib.uvad_sampler_state_bytes(C.byref(cfg), R, len(sup), D)), 256), dtype=torch.uint8,
                                       device=self.device)}
            self._check(self.lib.uvad_sampler_reset(
                self.ctx, st["state"].data_ptr(), st["state"].numel(), C.byref(cfg), pcm.data_ptr(), fmt, first.ctypes.data_as(C.POINTER(C.c_int64)),
                R, sup.ctypes.data_as(C.POINTER(C.c_int64)) if len(sup) else None, sup_first.ctypes.data_as(C.POINTER(C.c_int32)), len(sup),
                rec_set.ctypes.data_as(C.POINTER(C.c_int32)), w.ctypes.data_as(C.POINTER(C.c_double)), D, self._stream()))
            return st

    def sampler_step(self, st, B: int, out=None, labels=None, plan=False, cursor=None, draw=None, row0: int = 0):
        """One batch of B rows (uvad_sampler_step) -> dict(pcm (B, W) f32, nsamp (B,) int64, labels (B, T) uint8, frames (B,) int32, and
        plan (B, 8) int32 when asked for).  out / labels: the tensors to write (row strides of at least W / T elements; None: the
        handle's own per batch size, overwritten by the next step of that size); plan: True, or the tensor to write.  cursor and draw:
        an explicit position (uvad_sampler_apply: no state update), with row0 the index the first row draws under.  After the first call
        with a batch size nothing is allocated: the call can be captured."""
        B = int(B)
        with torch.cuda.device(self.device):
            buf = st["bufs"].get(B)
            if buf is None:
                buf = st["bufs"][B] = {"pcm": torch.zeros((B, st["W"]), dtype=torch.float32, device=self.device),
                                       "labels": torch.zeros((B, st["T"]), dtype=torch.uint8, device=self.device),
                                       "nsamp": torch.zeros(B, dtype=torch.int64, device=self.device),
                                       "frames": torch.zeros(B, dtype=torch.int32, device=self.device),
                                       "plan": torch.zeros((B, _lib.SAMPLER_PLAN_WORDS), dtype=torch.int32, device=self.device)}
            out = buf["pcm"] if out is None else out
            labels = buf["labels"] if labels is None else labels
            for t, dt, w, name in ((out, torch.float32, st["W"], "out"), (labels, torch.uint8, st["T"], "labels")):
                if not (torch.is_tensor(t) and t.device == self.device and t.dtype == dt and t.dim() == 2 and t.shape[0] == B and t.shape[1] >= w and
                        t.stride(1) == 1 and t.stride(0) >= t.shape[1]):
                    raise ValueError(f"{name} must be a ({B}, >= {w}) {dt} tensor on {self.device} with unit column stride")
            if plan is True:
                plan = buf["plan"]
            elif plan is False:
                plan = None
            elif not (torch.is_tensor(plan) and plan.device == self.device and plan.dtype == torch.int32 and
                      tuple(plan.shape) == (B, _lib.SAMPLER_PLAN_WORDS) and plan.is_contiguous()):
                raise ValueError(f"plan must be a contiguous int32 tensor of shape ({B}, {_lib.SAMPLER_PLAN_WORDS}) on {self.device}")
            need = int(self.lib.uvad_sampler_ws_bytes(B))
            if st["ws"] is None or st["ws"].numel() < need:
                st["ws"] = torch.zeros(need, dtype=torch.uint8, device=self.device)
            head = (self.ctx, B, out.data_ptr(), out.stride(0), buf["nsamp"].data_ptr(), labels.data_ptr(), labels.stride(0), buf["frames"].data_ptr(),
                    None if plan is None else plan.data_ptr())
            tail = (st["state"].data_ptr(), st["state"].numel(), st["ws"].data_ptr(), st["ws"].numel(), self._stream())
            if cursor is None and draw is None:
                self._check(self.lib.uvad_sampler_step(*head, *tail))
            else:
                if cursor is None or draw is None:
                    raise ValueError("cursor and draw go together (uvad_sampler_apply)")
                cur = np.ascontiguousarray(np.broadcast_to(np.asarray(cursor, np.int64), (st["D"],)))
                self._check(self.lib.uvad_sampler_apply(*head, cur.ctypes.data_as(C.POINTER(C.c_int64)), int(row0), int(draw) & 0xFFFFFFFFFFFFFFFF, *tail))
            res = {"pcm": out, "nsamp": buf["nsamp"], "labels": labels, "frames": buf["frames"]}
            if plan is not None:
                res["plan"] = plan
            return res

    def sampler_read(self, st) -> np.ndarray:
        """The record {draw ordinal, cursor of every dataset} (1 + D int64) of uvad_sampler_read, on the host (synchronises)."""
        with torch.cuda.device(self.device):
            rec = torch.zeros(1 + st["D"], dtype=torch.int64, device=self.device)
            self._check(self.lib.uvad_sampler_read(self.ctx, st["state"].data_ptr(), st["state"].numel(), rec.data_ptr(), self._stream()))
            return rec.cpu().numpy()

    def sampler_write(self, st, record):
        """Set the record sampler_read returned (uvad_sampler_write): the next step continues where that state stood."""
        rec = np.ascontiguousarray(record, np.int64).reshape(-1)
        if rec.shape != (1 + st["D"],):
            raise ValueError(f"the record holds 1 + D = {1 + st['D']} words")
        with torch.cuda.device(self.device):
            dev = torch.from_numpy(rec).to(self.device)
            self._check(self.lib.uvad_sampler_write(self.ctx, st["state"].data_ptr(), st["state"].numel(), dev.data_ptr(), self._stream()))
            torch.cuda.current_stream(self.device).synchronize()     # `dev` is freed on return

    def _lstm_train_ws(self, h, B: int, T: int):
        self._train_configure(h)
        need = int(self.lib.uvad_lstm_train_ws_bytes(self.ctx, B, T))
        if h["ws"] is None or h["ws"].numel() < need:
            h["ws"] = torch.zeros(need, dtype=torch.uint8, device=self.device)

    def lstm_train_forward(self, h, x_in: "torch.Tensor", lengths=None) -> "torch.Tensor":
        """The trainable layers' forward pass with the state's master weights (uvad_lstm_train_forward), keeping the activations in the
        handle's workspace: x_in (B, T, Din) from lstm_train_input -> y (B, T, hidden x directions), what head_train_grad takes as x.
        No copy to the host and no synchronisation."""
        with torch.cuda.device(self.device):
            x_in = self._dev_f32(x_in, "x_in")
            B, T, Din = x_in.shape
            want = self._lstm_train_shape(h["first_layer"])[0]
            if Din != want:
                raise ValueError(f"x_in has {Din} columns, layer {h['first_layer']} takes {want}")
            n = None if lengths is None else self._dev_lens(lengths, B, T, torch.int32, "lengths (frames)")
            self._lstm_train_ws(h, B, T)
            y = torch.empty((B, T, self._mc_c.hidden * (2 if self._mc_c.bidirectional else 1)), dtype=torch.float32, device=self.device)
            self._check(self.lib.uvad_lstm_train_forward(self.ctx, x_in.data_ptr(), B, T, n.data_ptr() if n is not None else None, y.data_ptr(),
                                                         h["state"].data_ptr(), h["state"].numel(), h["ws"].data_ptr(), h["ws"].numel(), self._stream()))
            h["_keep"] = (x_in, n, y)
            return y

    def lstm_train_backward(self, h, x_in: "torch.Tensor", dy: "torch.Tensor", lengths=None, want_grad_in: bool = False):
        """Backpropagation through time from dy (B, T, hidden x directions), head_train_grad's grad_x, through the activations the last
        lstm_train_forward of this handle kept (uvad_lstm_train_backward): adds the gradients and the frame count into the state.
        -> grad_in (B, T, Din) | None."""
        with torch.cuda.device(self.device):
            x_in, dy = self._dev_f32(x_in, "x_in"), self._dev_f32(dy, "dy")
            B, T, _ = x_in.shape
            if tuple(dy.shape) != (B, T, self._mc_c.hidden * (2 if self._mc_c.bidirectional else 1)):
                raise ValueError(f"dy has shape {tuple(dy.shape)}")
            n = None if lengths is None else self._dev_lens(lengths, B, T, torch.int32, "lengths (frames)")
            self._lstm_train_ws(h, B, T)
            g = torch.empty_like(x_in) if want_grad_in else None
            self._check(self.lib.uvad_lstm_train_backward(self.ctx, x_in.data_ptr(), dy.data_ptr(), B, T, n.data_ptr() if n is not None else None,
                                                          g.data_ptr() if g is not None else None, h["state"].data_ptr(), h["state"].numel(),
                                                          h["ws"].data_ptr(), h["ws"].numel(), self._stream()))
            h["_keep_b"] = (x_in, dy, n, g)
            return g

    def lstm_train_apply(self, h):
        """One Adam step from the accumulated gradients divided by the accumulated frame count (uvad_lstm_train_apply)."""
        self._train_apply(h)

    def lstm_train_read(self, h) -> dict:
        """Copy the state to the host (synchronises) -> {"weights", "grad", "m", "v": {torch key: tensor}, "frames", "step",
        "bias_correction1", "bias_correction2" (1 - beta^step), "draws" (the dropout draw ordinal), "scalars" (the raw record)}."""
        out, w = self._train_read(h)
        out["draws"] = int(w[8:10].view(np.uint64)[0])
        return out

    def lstm_train_state_dict(self, h) -> dict:
        """The adapted LSTM tensors keyed by torch key, ready to merge into a checkpoint (synchronises)."""
        return self.lstm_train_read(h)["weights"]

    def lstm_train_commit(self, h):
        """Make this runtime serve the adapted layers (uvad_lstm_train_commit: synchronises, re-finalizes).  Graphs captured before are
        stale, as after load_state_dict; the frozen prefix's sibling context is untouched."""
        self._train_commit(h)

    # ------------------------------------------------------------------ SincNet training (uvad_sincnet_train_*)
    def sincnet_train_keys(self, first_stage: int = 0):
        """[(torch key, shape)] of the learning tensors of stages first_stage .. 2 in the packed order of uvad_sincnet_train_read
        (state_dict order), with the model's ``sincnet.`` prefix."""
        q = self._sn_c
        nf, c2, c3 = q.n_filters, q.c2, q.c3
        every = [(0, "wav_norm1d.weight", (1,)), (0, "wav_norm1d.bias", (1,)), (0, "conv1d.0.filterbank.low_hz_", (nf // 2, 1)),
                 (0, "conv1d.0.filterbank.band_hz_", (nf // 2, 1)), (1, "conv1d.1.weight", (c2, nf, q.k2)), (1, "conv1d.1.bias", (c2,)),
                 (2, "conv1d.2.weight", (c3, c2, q.k3)), (2, "conv1d.2.bias", (c3,)), (0, "norm1d.0.weight", (nf,)), (0, "norm1d.0.bias", (nf,)),
                 (1, "norm1d.1.weight", (c2,)), (1, "norm1d.1.bias", (c2,)), (2, "norm1d.2.weight", (c3,)), (2, "norm1d.2.bias", (c3,))]
        return [("sincnet." + k, shape) for stage, k, shape in every if stage >= int(first_stage)]

    def sincnet_train_open(self, first_stage: int = 0, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, segment: int = 0):
        """Allocate and reset a training state for stages first_stage .. 2 of the SincNet front end (uvad_sincnet_train_reset): f32 master
        copies of their tensors as loaded (the band edges of the sinc bank among them), Adam moments, the gradient accumulator, the bank.
        segment: conv positions per gradient partial (0 = the library's default).  The handle owns the state and the workspace."""
        if self._sn_c is None:
            raise RuntimeError("this runtime has no SincNet stage")
        first_stage = int(first_stage)
        if not 0 <= first_stage <= 2:
            raise ValueError("first_stage must lie in 0 .. 2")
        cfg = _lib.SincNetTrainCfg(float(lr), float(betas[0]), float(betas[1]), float(eps), int(segment), first_stage)
        with torch.cuda.device(self.device):
            self._check(self.lib.uvad_sincnet_train_configure(self.ctx, C.byref(cfg)))
            P = int(self.lib.uvad_sincnet_train_param_count(self.ctx))
            h = {"family": "sincnet", "cfg": cfg, "P": P, "first_stage": first_stage, "ws": None,
                 "state": torch.empty(int(self.lib.uvad_sincnet_train_state_bytes(self.ctx)), dtype=torch.uint8, device=self.device),
                 "out": torch.zeros(max(P, _lib.HEAD_TRAIN_SCALAR_WORDS, self._sn_c.n_filters * self._sn_c.kernel_size), dtype=torch.float32,
                                    device=self.device)}
            self._check(self.lib.uvad_sincnet_train_reset(self.ctx, h["state"].data_ptr(), h["state"].numel(), self._stream()))
            return h

    def _sincnet_train_wav(self, wav: "torch.Tensor") -> "torch.Tensor":
        wav = self._dev_f32(wav, "wav")
        if wav.dim() == 3:
            if wav.shape[1] != 1:
                raise ValueError(f"Only single channel is supported. You have {wav.shape[1]}")
            wav = wav[:, 0, :].contiguous()
        if wav.dim() != 2:
            raise ValueError("wav must be (B, S) or (B, 1, S)")
        return wav

    def _sincnet_train_ws(self, h, B: int, S: int):
        self._train_configure(h)
        need = int(self.lib.uvad_sincnet_train_ws_bytes(self.ctx, B, S))
        if need == 0:
            raise ValueError(f"uvad_sincnet_train does not serve B = {B}, S = {S} (at least one frame; B x L_0 <= 2^31 - 1; <= 65535 segments)")
        if h["ws"] is None or h["ws"].numel() < need:
            h["ws"] = torch.zeros(need, dtype=torch.uint8, device=self.device)

    def sincnet_train_forward(self, h, wav: "torch.Tensor") -> "torch.Tensor":
        """The front end's forward pass with the state's master weights (uvad_sincnet_train_forward), keeping the activations in the
        handle's workspace: wav (B, S) or (B, 1, S) f32 on the GPU -> feats (B, T, c3), what lstm_train_forward takes as x_in.  No copy
        to the host and no synchronisation."""
        with torch.cuda.device(self.device):
            wav = self._sincnet_train_wav(wav)
            B, S = wav.shape
            self._sincnet_train_ws(h, B, S)
            T = int(self.lib.uvad_sincnet_num_frames(self.ctx, S))
            feats = torch.empty((B, T, self._sn_c.c3), dtype=torch.float32, device=self.device)
            self._check(self.lib.uvad_sincnet_train_forward(self.ctx, wav.data_ptr(), B, S, feats.data_ptr(), h["state"].data_ptr(), h["state"].numel(),
                                                            h["ws"].data_ptr(), h["ws"].numel(), self._stream()))
            h["_keep"] = (wav, feats)
            return feats

    def sincnet_train_backward(self, h, wav: "torch.Tensor", dfeats: "torch.Tensor"):
        """The backward pass from dfeats (B, T, c3), lstm_train_backward's grad_in (the gradient of the summed loss), through the
        activations the last sincnet_train_forward of this handle kept (uvad_sincnet_train_backward): adds the gradients and the B T
        frames into the state."""
        with torch.cuda.device(self.device):
            wav, dfeats = self._sincnet_train_wav(wav), self._dev_f32(dfeats, "dfeats")
            B, S = wav.shape
            T = int(self.lib.uvad_sincnet_num_frames(self.ctx, S))
            if tuple(dfeats.shape) != (B, T, self._sn_c.c3):
                raise ValueError(f"dfeats has shape {tuple(dfeats.shape)}, expected {(B, T, self._sn_c.c3)}")
            self._sincnet_train_ws(h, B, S)
            self._check(self.lib.uvad_sincnet_train_backward(self.ctx, wav.data_ptr(), dfeats.data_ptr(), B, S, h["state"].data_ptr(),
                                                             h["state"].numel(), h["ws"].data_ptr(), h["ws"].numel(), self._stream()))
            h["_keep_b"] = (wav, dfeats)

    def sincnet_train_apply(self, h):
        """One Adam step from the accumulated gradients divided by the accumulated frame count (uvad_sincnet_train_apply)."""
        self._train_apply(h)

    def sincnet_train_read(self, h) -> dict:
        """Copy the state to the host (synchronises) -> {"weights", "grad", "m", "v": {torch key: tensor}, "filters" (the bank of the last
        forward call, (n_filters, kernel_size)), "frames", "step", "bias_correction1", "bias_correction2" (1 - beta^step), "scalars"}."""
        out, _ = self._train_read(h)
        nf, ks = self._sn_c.n_filters, self._sn_c.kernel_size
        with torch.cuda.device(self.device):   # the context is still configured from h
            out["filters"] = torch.from_numpy(self._train_block(h, _lib.SINCNET_TRAIN_FILTERS)[:nf * ks].reshape(nf, ks).copy())
        return out

    def sincnet_train_state_dict(self, h) -> dict:
        """The adapted SincNet tensors keyed by torch key (reference names, ``sincnet.`` prefix), ready to merge into a checkpoint
        (synchronises)."""
        return self.sincnet_train_read(h)["weights"]

    def sincnet_train_commit(self, h):
        """Make this runtime serve the adapted front end (uvad_sincnet_train_commit: synchronises, re-finalizes; the bank served is the one
        the last forward call ran).  Graphs captured before are stale, as after load_state_dict."""
        self._train_commit(h)

    # ------------------------------------------------------------------ the joint optimizer step (uvad_optim_*) and the _write calls
    def optim_open(self, cfg=None, lr_table=(1e-3,)):
        """Allocate and reset an optimizer state (uvad_optim_reset).  cfg: {"betas": (0.9, 0.999), "eps": 1e-8, "max_norm": 0 (no
        clipping), "weight_decay": 0, "adamw": False (L2 into the gradient; True: decoupled), "skip_nonfinite": False, "lr_scale": (1, 1, 1)
        for head, LSTM, SincNet}.  lr_table: the learning rate of applied step t is lr_table[min(t, len - 1)], rounded to f32 here.  The
        handle owns the state and the workspace."""
        cfg = dict(cfg or {})
        known = {"betas", "eps", "max_norm", "weight_decay", "adamw", "skip_nonfinite", "lr_scale"}
        if set(cfg) - known:
            raise ValueError(f"optim_open: unknown option(s) {sorted(set(cfg) - known)}")
        betas, scale = cfg.get("betas", (0.9, 0.999)), tuple(cfg.get("lr_scale", (1.0, 1.0, 1.0)))
        if len(scale) != 3:
            raise ValueError("lr_scale needs three entries: head, LSTM, SincNet")
        q = _lib.OptimCfg(float(betas[0]), float(betas[1]), float(cfg.get("eps", 1e-8)), float(cfg.get("max_norm", 0.0) or 0.0),
                          float(cfg.get("weight_decay", 0.0) or 0.0), int(bool(cfg.get("adamw", False))), int(bool(cfg.get("skip_nonfinite", False))),
                          (C.c_float * 3)(*[float(v) for v in scale]))
        table = np.ascontiguousarray(np.asarray(lr_table, np.float64).reshape(-1).astype(np.float32))
        with torch.cuda.device(self.device):
            o = {"cfg": q, "n": int(table.size), "ws": None, "table": table,
                 "state": torch.zeros(max(int(self.lib.uvad_optim_state_bytes(int(table.size))), 256), dtype=torch.uint8, device=self.device),
                 "out": torch.zeros(_lib.OPTIM_RECORD_WORDS, dtype=torch.int32, device=self.device)}
            self._check(self.lib.uvad_optim_reset(self.ctx, o["state"].data_ptr(), o["state"].numel(), C.byref(q),
                                                  table.ctypes.data_as(C.POINTER(C.c_float)), int(table.size), self._stream()))
            return o

    def optim_set_lr(self, o, table):
        """Rewrite the learning-rate table between steps (uvad_optim_set_lr_table): at most optim_open's entry count; a captured graph
        picks the new values up on its next replay.  Synchronises the stream."""
        table = np.ascontiguousarray(np.asarray(table, np.float64).reshape(-1).astype(np.float32))
        with torch.cuda.device(self.device):
            self._check(self.lib.uvad_optim_set_lr_table(self.ctx, o["state"].data_ptr(), o["state"].numel(),
                                                         table.ctypes.data_as(C.POINTER(C.c_float)), int(table.size), self._stream()))
        o["table"] = table

    def optim_step(self, o, head=None, lstm=None, sincnet=None):
        """One joint step over the handles given (uvad_optim_step) in place of their _apply calls: the global gradient norm, clipping,
        weight decay, the table's learning rate, Adam; no copy to the host and no synchronisation, so once the workspace exists the call
        can be captured."""
        if head is None and lstm is None and sincnet is None:
            raise ValueError("optim_step needs at least one training handle")
        with torch.cuda.device(self.device):
            for h in (head, lstm, sincnet):
                if h is not None:
                    self._train_configure(h)
            need = int(self.lib.uvad_optim_ws_bytes(self.ctx))
            if o["ws"] is None or o["ws"].numel() < need:
                o["ws"] = torch.zeros(need, dtype=torch.uint8, device=self.device)
            arg = lambda h: (h["state"].data_ptr(), h["state"].numel()) if h is not None else (None, 0)
            self._check(self.lib.uvad_optim_step(self.ctx, *arg(head), *arg(lstm), *arg(sincnet), o["state"].data_ptr(), o["state"].numel(),
                                                 o["ws"].data_ptr(), o["ws"].numel(), self._stream()))

    def optim_read(self, o) -> dict:
        """The record of the last step and the counts (uvad_optim_read; synchronises) -> {"norm", "coef", "lr" (of the last step that had
        a participant), "took_part": (head, LSTM, SincNet), "step" (applied steps), "skipped", "record": the raw words, an int32 tensor}."""
        with torch.cuda.device(self.device):
            self._check(self.lib.uvad_optim_read(self.ctx, o["state"].data_ptr(), o["state"].numel(), o["out"].data_ptr(), self._stream()))
            w = o["out"].cpu().numpy().copy()
        f, u = w.view(np.float32), w.view(np.uint32)
        return {"norm": float(f[0]), "coef": float(f[1]), "lr": float(f[2]), "took_part": tuple(bool(int(u[3]) >> k & 1) for k in range(3)),
                "step": int(u[4:6].view(np.uint64)[0]), "skipped": int(u[6:8].view(np.uint64)[0]), "record": torch.from_numpy(w)}

    def optim_write(self, o, record):
        """Put back what optim_read returned (its dict or its "record" tensor; uvad_optim_write): the counts and the last step's record."""
        rec = record["record"] if isinstance(record, dict) else record
        with torch.cuda.device(self.device):
            src = torch.as_tensor(rec).to(torch.int32).reshape(-1)[:_lib.OPTIM_RECORD_WORDS].contiguous().to(self.device)
            self._check(self.lib.uvad_optim_write(self.ctx, o["state"].data_ptr(), o["state"].numel(), src.data_ptr(), self._stream()))
            o["_keep_w"] = src

    def _train_write(self, h, st):
        """The _write companion of a family's _read: st["weights"], st["m"], st["v"] ({torch key: tensor}) and st["scalars"] (the raw words)."""
        fn, keys = self._train_fn(h, "write"), self._TRAIN_FAMILIES[h["family"]][0](self, h)
        with torch.cuda.device(self.device):
            self._train_configure(h)
            keep = []
            for name, which in (("weights", _lib.HEAD_TRAIN_MASTERS), ("m", _lib.HEAD_TRAIN_M), ("v", _lib.HEAD_TRAIN_V)):
                if st.get(name) is None:
                    continue
                parts = []
                for key, shape in keys:
                    t = torch.as_tensor(st[name][key]).detach().to(torch.float32).cpu()
                    if tuple(t.shape) != tuple(shape):
                        raise ValueError(f"{name}[{key}] has shape {tuple(t.shape)}, expected {tuple(shape)}")
                    parts.append(t.reshape(-1))
                flat = torch.cat(parts).contiguous().to(self.device)
                self._check(fn(self.ctx, h["state"].data_ptr(), h["state"].numel(), which, flat.data_ptr(), self._stream()))
                keep.append(flat)
            if st.get("scalars") is not None:
                words = torch.zeros(_lib.LSTM_TRAIN_SCALAR_WORDS, dtype=torch.int32)
                src = torch.as_tensor(st["scalars"]).to(torch.int32).reshape(-1)
                words[:src.numel()] = src[:words.numel()]
                words = words.to(self.device)
                self._check(fn(self.ctx, h["state"].data_ptr(), h["state"].numel(), _lib.HEAD_TRAIN_SCALARS, words.data_ptr(), self._stream()))
                keep.append(words)
            h["_keep_w"] = keep          # the launches read them after this call returns

    def head_train_write(self, h, st):
        """Put back what head_train_read returned (uvad_head_train_write): masters, m, v, and from "scalars" the step and the bias
        corrections.  The accumulated gradient, loss and frames are not written: a write belongs between steps."""
        self._train_write(h, st)

    def lstm_train_write(self, h, st):
        """head_train_write for an LSTM handle (uvad_lstm_train_write); "scalars" carries the dropout draw ordinal as well."""
        self._train_write(h, st)

    def sincnet_train_write(self, h, st):
        """head_train_write for a SincNet handle (uvad_sincnet_train_write); the bank is rebuilt from the masters by the next forward call."""
        self._train_write(h, st)

    # ------------------------------------------------------------------ scoring against reference labels (uvad_score_*)
    def score_open(self, points=((0.5, 25),), collar: int = 0, bins: int = 256, segment: int = 0):
        """Allocate and reset a scoring state (uvad_score_reset): points [(threshold, odd median kernel)], 1 .. 8 of them; collar frames
        left unscored around every reference boundary; bins of the threshold sweep (a power of two); segment: frames per workgroup
        (0 = the library's default; no output depends on it)."""
        points = [(float(t), int(k)) for t, k in points]
        if not 1 <= len(points) <= _lib.SCORE_MAX_POINTS:
            raise ValueError(f"need 1 .. {_lib.SCORE_MAX_POINTS} operating points, got {len(points)}")
        cfg = _lib.ScoreCfg()
        cfg.n_points, cfg.collar, cfg.bins, cfg.segment = len(points), int(collar), int(bins), int(segment)
        for m, (t, k) in enumerate(points):
            cfg.threshold[m], cfg.kernel[m] = t, k
        with torch.cuda.device(self.device):
            self._check(self.lib.uvad_score_configure(self.ctx, C.byref(cfg)))
            nbytes = int(self.lib.uvad_score_state_bytes(self.ctx))
            sc = {"cfg": cfg, "points": points, "collar": int(collar), "bins": int(bins),
                  "state": torch.empty(nbytes, dtype=torch.uint8, device=self.device), "ws": None, "rows": None,
                  "totals": torch.zeros(_lib.SCORE_TOTALS_WORDS, dtype=torch.int64, device=self.device)}
            self.score_reset(sc)
            return sc

    def score_reset(self, sc):
        """Empty the accumulated totals (uvad_score_reset)."""
        with torch.cuda.device(self.device):
            self._check(self.lib.uvad_score_configure(self.ctx, C.byref(sc["cfg"])))   # host only: the context serves any number of scorers
            self._check(self.lib.uvad_score_reset(self.ctx, sc["state"].data_ptr(), sc["state"].numel(), self._stream()))

    @staticmethod
    def _rows_2d(t, dtype, name):
        if t.dim() != 2 or t.dtype != dtype or (t.shape[1] > 1 and t.stride(1) != 1) or t.stride(0) < t.shape[1]:
            raise ValueError(f"{name} must be a (B, T) {dtype} tensor with contiguous rows")
        return t

    def score_step(self, sc, probs: "torch.Tensor", gt: "torch.Tensor", lengths=None, rows: bool = False):
        """Accumulate one batch (uvad_score_step): probs (B, T) f32 and gt (B, T) uint8 (non-zero = speech) on the GPU -- row-strided views
        are used as they are -- and lengths (B,) valid frames per row (a device int32 tensor is read on the device).  No copy to the host
        and no synchronisation: once the workspace has the size of the batch shape (the first call with it allocates), the call can be
        captured into a graph.  rows=True returns this step's (B, 4) int64 {tp, fp, tn, fn} of operating point 0, on the device and
        overwritten by the next such step.  score_batch_loss gives the step's mean loss."""
        with torch.cuda.device(self.device):
            for t, name in ((probs, "probs"), (gt, "gt")):
                if not torch.is_tensor(t) or t.device != self.device:
                    raise RuntimeError(f"{name} must be a tensor on {self.device}")
            probs = self._rows_2d(probs, torch.float32, "probs")
            gt = self._rows_2d(gt, torch.uint8, "gt")
            B, T = probs.shape
            if tuple(gt.shape) != (B, T):
                raise ValueError(f"gt {tuple(gt.shape)} does not match probs {(B, T)}")
            n = None if lengths is None else self._dev_lens(lengths, B, T, torch.int32, "lengths (frames)")
            self._check(self.lib.uvad_score_configure(self.ctx, C.byref(sc["cfg"])))
            need = int(self.lib.uvad_score_ws_bytes(self.ctx, B, T))
            if sc["ws"] is None or sc["ws"].numel() < need:
                sc["ws"] = torch.zeros(max(need, 32), dtype=torch.uint8, device=self.device)
            out = None
            if rows:
                if sc["rows"] is None or sc["rows"].shape[0] < B:
                    sc["rows"] = torch.zeros((B, 4), dtype=torch.int64, device=self.device)
                out = sc["rows"][:B]
            self._check(self.lib.uvad_score_step(self.ctx, probs.data_ptr(), probs.stride(0), gt.data_ptr(), gt.stride(0), B, T,
                                                 n.data_ptr() if n is not None else None, sc["state"].data_ptr(), sc["state"].numel(),
                                                 out.data_ptr() if out is not None else None, sc["ws"].data_ptr(), sc["ws"].numel(),
                                                 self._stream()))
            sc["_keep"] = (probs, gt, n)   # the launch reads them after this call returns
            return out

    def score_batch_loss(self, sc) -> "torch.Tensor":
        """The most recent step's mean binary cross-entropy over its valid frames as a 0-d f64 tensor on the device (NaN when a valid
        probability is NaN, or when the step had no valid frame): what test_step returns, without a synchronisation."""
        head = sc["ws"][:16]
        return head[:8].view(torch.float64)[0] / head[8:].view(torch.int64)[0].to(torch.float64)

    def score_read(self, sc) -> dict:
        """Copy the accumulated totals to the host (uvad_score_totals; synchronises) -> {"points", "collar", "bins", "counts" (n_points, 4)
        int64 {tp, fp, tn, fn} pooled over the scored frames, "hist" (2, bins) int64 [class][bin], "loss_sum" float, "valid" frames,
        "steps"}: what postprocess.score_metrics and det_curve take."""
        with torch.cuda.device(self.device):
            self._check(self.lib.uvad_score_totals(self.ctx, sc["state"].data_ptr(), sc["state"].numel(), sc["totals"].data_ptr(), self._stream()))
            w = sc["totals"].cpu().numpy()
        npts, bins = int(w[0]), int(w[1])
        return {"points": list(sc["points"]), "collar": sc["collar"], "bins": bins,
                "counts": w[8:8 + 4 * npts].reshape(npts, 4).copy(),
                "hist": np.stack([w[40:40 + bins], w[40 + 1024:40 + 1024 + bins]]).copy(),
                "loss_sum": float(w[3:4].view(np.float64)[0]), "valid": int(w[2]), "steps": int(w[4])}

    def intervals_to_labels(self, intervals, counts, T: int, lengths=None, out=None) -> "torch.Tensor":
        """Reference intervals -> label rows on the device (uvad_intervals_to_labels): intervals (B, max_iv, 2) int32 {start, end} frames and
        counts (B,) int32, tensors on the GPU or anything numpy converts; lengths (B,) valid frames per row.  -> (B, T) uint8, 1 on the
        union of the row's intervals inside [0, len), 0 elsewhere on it.  out: a (B, >= T) uint8 tensor with contiguous rows to write
        into -- its bytes at or past each row's length are left as they are; without it a zeroed tensor is made."""
        with torch.cuda.device(self.device):
            iv = intervals if torch.is_tensor(intervals) else torch.from_numpy(np.ascontiguousarray(intervals, np.int32))
            iv = iv.to(self.device, torch.int32).contiguous()
            if iv.dim() != 3 or iv.shape[2] != 2:
                raise ValueError(f"intervals must be (B, max_iv, 2), got {tuple(iv.shape)}")
            B, max_iv = int(iv.shape[0]), int(iv.shape[1])
            cn = counts if torch.is_tensor(counts) else torch.from_numpy(np.ascontiguousarray(counts, np.int32))
            cn = cn.to(self.device, torch.int32).contiguous()
            if tuple(cn.shape) != (B,):
                raise ValueError(f"counts must be ({B},), got {tuple(cn.shape)}")
            if out is None:
                out = torch.zeros((B, T), dtype=torch.uint8, device=self.device)
            elif not torch.is_tensor(out) or out.device != self.device or out.shape[0] != B:
                raise ValueError(f"out must be a ({B}, >= {T}) uint8 tensor on {self.device}")
            out = self._rows_2d(out, torch.uint8, "out")
            n = None if lengths is None else self._dev_lens(lengths, B, T, torch.int32, "lengths (frames)")
            self._check(self.lib.uvad_intervals_to_labels(self.ctx, iv.data_ptr() if max_iv else None, cn.data_ptr(), B, max_iv, int(T),
                                                          out.stride(0), n.data_ptr() if n is not None else None, out.data_ptr(),
                                                          self._stream()))
            return out[:, :T]

    # ------------------------------------------------------------------ speech cuts (uvad_cuts_*)
    def cuts_open(self, pad: int = 0, max_len: int = 0, min_len: int = 0, hop: int = 160, lead: int = 0, tail: int = 240, max_cuts=None):
        """The configuration and the buffers of the cut calls below: runs widened by `pad` frames and merged, split into pieces of at
        most `max_len` frames (0: no splitting) whose last piece is dropped when it has `min_len` frames or fewer; `hop` samples per
        frame, `lead` / `tail` samples taken before the first frame and past the last frame's hop (postprocess.cuts_config makes these
        from the reference's seconds).  max_cuts: rows of the table and of the gathered batch (default: B x uvad_cuts_max_per_row, which
        never overflows).  Buffers are sized by the first call with a shape; after that the calls allocate nothing and can be captured."""
        cfg = _lib.CutsCfg(int(pad), int(max_len), int(min_len), int(hop), int(lead), int(tail))
        if int(self.lib.uvad_cuts_max_per_row(C.byref(cfg), 1)) == 0:
            raise ValueError(f"bad cuts configuration: pad {pad} (0 .. 2^20), max_len {max_len} (0 .. 2^24), min_len {min_len} (>= 0, < max_len "
                             f"when splitting), hop {hop} (>= 1), lead {lead} and tail {tail} (>= 0)")
        if max_cuts is not None and int(max_cuts) < 0:
            raise ValueError("max_cuts must be >= 0")
        return {"cfg": cfg, "max_cuts": None if max_cuts is None else int(max_cuts), "table": None, "row_first": None,
                "total": torch.zeros(1, dtype=torch.int32, device=self.device), "ws": None, "out": {}, "out_len": None}

    def cuts_table(self, labels: "torch.Tensor", lengths=None, nsamp=None, S=None, cuts=None, **cfg):
        """labels (B, T) uint8 on the GPU (non-zero = speech; row-strided views are used as they are), lengths (B,) valid frames and nsamp
        (B,) samples per row (device tensors are read on the device), S: samples per row of the audio the cuts will be taken from
        (default: the largest nsamp, or T * hop + tail).  cuts: a state of cuts_open; without it one is opened from **cfg.
        -> (table (max_cuts, 8) int32 -- uvad_cut rows {row, index, first_frame, n_frames, first_sample lo / hi, n_samples lo / hi} --,
        row_first (B + 1,) int32, total (1,) int32), on the device and overwritten by the next call on the state.  cuts_read gives the
        host view."""
        ct = cuts if cuts is not None else self.cuts_open(**cfg)
        with torch.cuda.device(self.device):
            if not torch.is_tensor(labels) or labels.device != self.device:
                raise RuntimeError(f"labels must be a tensor on {self.device}")
            labels = self._rows_2d(labels, torch.uint8, "labels")
            B, T = labels.shape
            q = ct["cfg"]
            n = None if lengths is None else self._dev_lens(lengths, B, T, torch.int32, "lengths (frames)")
            if S is None:
                S = int(max(nsamp.tolist() if torch.is_tensor(nsamp) else nsamp)) if nsamp is not None else T * q.hop + q.tail
            ns = None if nsamp is None else self._dev_lens(nsamp, B, int(S), torch.int64, "nsamp (samples)")
            per_row = int(self.lib.uvad_cuts_max_per_row(C.byref(q), T))
            if ct["max_cuts"] is None:
                ct["max_cuts"] = B * per_row
            mc = ct["max_cuts"]
            if ct["table"] is None:
                ct["table"] = torch.zeros((max(mc, 1), 8), dtype=torch.int32, device=self.device)
                ct["out_len"] = torch.zeros(max(mc, 1), dtype=torch.int32, device=self.device)
            if ct["row_first"] is None or ct["row_first"].numel() != B + 1:
                ct["row_first"] = torch.zeros(B + 1, dtype=torch.int32, device=self.device)
            need = int(self.lib.uvad_cuts_ws_bytes(self.ctx, B, T))
            if ct["ws"] is None or ct["ws"].numel() < need:
                ct["ws"] = torch.zeros(max(need, 16), dtype=torch.uint8, device=self.device)
            self._check(self.lib.uvad_cuts_table(self.ctx, labels.data_ptr(), labels.stride(0) if B > 1 else max(labels.stride(0), T), B, T,
                                                 n.data_ptr() if n is not None else None, ns.data_ptr() if ns is not None else None, int(S),
                                                 C.byref(q), ct["table"].data_ptr() if mc else None, mc, ct["row_first"].data_ptr(),
                                                 ct["total"].data_ptr(), ct["ws"].data_ptr(), ct["ws"].numel(), self._stream()))
            ct["_keep"] = (labels, n, ns)   # the launch reads them after this call returns
            ct["S"] = int(S)
            return ct["table"][:mc], ct["row_first"], ct["total"]

    def cuts_gather(self, src: "torch.Tensor", cuts, which: str = "samples", ld_out=None, rows=None, table=None):
        """The audio (which="samples": src (B, S) int16 or f32) or the feature frames (which="frames": src (B, T, F) f32) of the cuts the
        last cuts_table on the state `cuts` listed -> (batch (max_cuts, ld_out[, F]) of src's type, lengths (max_cuts,) int32): row i <
        total holds the cut's first min(n, ld_out) units, then zeros; later rows are left as they are.  ld_out defaults to
        uvad_cuts_max_samples rounded up to 8 (samples) or the longest possible cut in frames; rows (default max_cuts) bounds the
        batch's rows: the batch is rows x ld_out units of memory whatever the labels hold, so a caller who knows the total (cuts_read)
        or an upper bound passes it, here or as cuts_open's max_cuts.  table: another table of the same cuts to gather by (fuse_pick's,
        whose rows are the picked channels' rows of src); default: the state's own."""
        ct = cuts
        if ct.get("table") is None:
            raise RuntimeError("cuts_gather needs a state on which cuts_table has run")
        if which not in ("samples", "frames"):
            raise ValueError(f"which must be 'samples' or 'frames', got {which!r}")
        with torch.cuda.device(self.device):
            if not torch.is_tensor(src) or src.device != self.device:
                raise RuntimeError(f"src must be a tensor on {self.device}")
            q = ct["cfg"]
            if which == "samples":
                if src.dim() != 2 or src.dtype not in (torch.int16, torch.float32) or (src.shape[1] > 1 and src.stride(1) != 1):
                    raise ValueError("samples: src must be a (B, S) int16 or float32 tensor with contiguous rows")
                unit, tailshape, row_stride = src.element_size(), (), src.stride(0) if src.shape[0] > 1 else max(src.stride(0), src.shape[1])
                if ld_out is None:
                    ld_out = -(-int(self.lib.uvad_cuts_max_samples(C.byref(q), src.shape[1])) // 8) * 8
            else:
                if src.dim() != 3 or src.dtype != torch.float32 or not src.is_contiguous():
                    raise ValueError("frames: src must be a contiguous (B, T, F) float32 tensor")
                unit, tailshape, row_stride = 4 * src.shape[2], (src.shape[2],), src.shape[1]
                if ld_out is None:
                    ld_out = q.max_len if q.max_len else src.shape[1]
            ld_out = max(int(ld_out), 1)
            mc = ct["max_cuts"] if rows is None else min(ct["max_cuts"], max(int(rows), 0))
            key = (which, src.dtype, ld_out, mc) + tailshape
            if key not in ct["out"]:
                ct["out"][key] = torch.zeros((max(mc, 1), ld_out) + tailshape, dtype=src.dtype, device=self.device)
            out = ct["out"][key]
            self._check(self.lib.uvad_cuts_gather(self.ctx, src.data_ptr(), row_stride, unit, _lib.CUTS_SAMPLES if which == "samples" else _lib.CUTS_FRAMES,
                                                  (ct["table"] if table is None else table).data_ptr(), ct["total"].data_ptr(), mc, out.data_ptr(), ld_out,
                                                  ct["out_len"].data_ptr(), self._stream()))
            ct["_keep_src"] = src
            return out[:mc], ct["out_len"][:mc]

    def speech_cuts(self, labels: "torch.Tensor", pcm: "torch.Tensor", lengths=None, nsamp=None, cuts=None, ld_out=None, **cfg):
        """Labels and the audio they were made from, both on the GPU -> (table, batch, lengths): cuts_table, then cuts_gather of the
        samples, with no copy to the host in between -- the padded batch a recogniser takes.  pcm (B, S) int16 or f32; see cuts_table
        and cuts_gather for the rest.  The state used is returned by neither: pass one from cuts_open to keep it (graphs, cuts_read)."""
        ct = cuts if cuts is not None else self.cuts_open(**cfg)
        table, _, _ = self.cuts_table(labels, lengths=lengths, nsamp=nsamp, S=int(pcm.shape[1]), cuts=ct)
        batch, lens = self.cuts_gather(pcm, ct, "samples", ld_out=ld_out)
        return table, batch, lens

    def cuts_read(self, cuts) -> np.ndarray:
        """The cuts the last cuts_table listed, copied to the host (synchronises): a structured array with uvad_cut's fields {row, index,
        first_frame, n_frames, first_sample, n_samples}, min(total, max_cuts) entries."""
        dt = np.dtype([("row", "<i4"), ("index", "<i4"), ("first_frame", "<i4"), ("n_frames", "<i4"), ("first_sample", "<i8"), ("n_samples", "<i8")])
        with torch.cuda.device(self.device):
            n = min(int(cuts["total"].cpu()[0]), cuts["max_cuts"])
            return cuts["table"][:n].cpu().numpy().view(dt).reshape(-1).copy()

    # ------------------------------------------------------------------ the cut-supervision join (uvad_cuts_join)
    JOIN_MODES = {"overlap": _lib.JOIN_OVERLAP, "inside": _lib.JOIN_INSIDE}
    # the reference's seven counters (predict.py:597-611) and the audit word each is; word 1, the cuts taking part, goes as "New cuts"
    JOIN_AUDIT_NAMES = (("Total Supervisions", 0), ("Supervisions in new cuts", 2), ("Unique Supervisions in new cuts", 3),
                        ("Supervisions not in new cuts", 4), ("Supervisions exceeding new cuts", 5),
                        ("Supervisions in multiple new cuts", 6), ("Empty cuts", 7), ("New cuts", 1))

    def cuts_join(self, cuts, intervals, counts, mode: str = "overlap", max_pairs=None, rows=None):
        """Which items belong to which cut (uvad_cuts_join), on a state of cuts_open after cuts_table, with no copy to the host: intervals
        (B, max_iv, 2) int32 {start, end} in frames and counts (B,) int32 -- one row per row of the labels, the layout of
        intervals_to_labels, so postprocess.supervision_frames feeds both; tensors on the GPU are read in place (a captured graph
        replays with new items), anything else is uploaded.  mode "overlap": an item matches every cut it shares a frame with (the
        supervisions of cut.truncate); "inside": the cut that holds it whole (the words of an alignment).
        max_pairs: slots of `pairs` (default: min(max_cuts x max_iv, max_cuts + B x max_iv), which holds every pair when a row's items
        do not overlap one another; pairs past it are counted, not stored, and pair_first's last used entry is the true total to retry with).
        rows (default max_cuts) bounds the cuts that take part, as in cuts_gather: a caller who knows the total (cuts_read) passes it, which
        keeps max_cuts x max_iv, what the call can count, small.
        -> {"pair_first" (max_cuts + 1,), "pairs" (max_pairs,), "item_cuts" (B, max_iv, 2) int32, "audit" (B + 1, 8) int64}: device
        tensors kept on the state and overwritten by the next call.  cuts_join_read gives the host view."""
        ct = cuts
        if ct.get("table") is None:
            raise RuntimeError("cuts_join needs a state on which cuts_table has run")
        if mode not in self.JOIN_MODES:
            raise ValueError(f"mode must be one of {sorted(self.JOIN_MODES)}, got {mode!r}")
        with torch.cuda.device(self.device):
            iv = intervals if torch.is_tensor(intervals) else torch.from_numpy(np.ascontiguousarray(intervals, np.int32))
            iv = iv.to(self.device, torch.int32).contiguous()
            if iv.dim() != 3 or iv.shape[2] != 2:
                raise ValueError(f"intervals must be (B, max_iv, 2), got {tuple(iv.shape)}")
            B, max_iv = int(iv.shape[0]), int(iv.shape[1])
            if B != ct["row_first"].numel() - 1:
                raise ValueError(f"intervals has {B} rows, the cut table was made from {ct['row_first'].numel() - 1}")
            cn = counts if torch.is_tensor(counts) else torch.from_numpy(np.ascontiguousarray(counts, np.int32))
            cn = cn.to(self.device, torch.int32).contiguous()
            if tuple(cn.shape) != (B,):
                raise ValueError(f"counts must be ({B},), got {tuple(cn.shape)}")
            mc = ct["max_cuts"] if rows is None else min(ct["max_cuts"], max(int(rows), 0))
            if mc * max_iv > 0x7fffffff:
                raise ValueError(f"max_cuts x max_iv = {mc * max_iv} is above 2^31 - 1: pass rows= (or cuts_open's max_cuts) near the total")
            mp = min(mc * max_iv, mc + B * max_iv) if max_pairs is None else int(max_pairs)
            if mp < 0:
                raise ValueError("max_pairs must be >= 0")
            key = (B, max_iv, mp, mc)
            jn = ct.get("join")
            if jn is None or jn["key"] != key:
                need = int(self.lib.uvad_cuts_join_ws_bytes(self.ctx, B, max_iv, mc))
                jn = ct["join"] = {"key": key,
                                   "pair_first": torch.zeros(mc + 1, dtype=torch.int32, device=self.device),
                                   "pairs": torch.zeros(max(mp, 1), dtype=torch.int32, device=self.device),
                                   "item_cuts": torch.zeros((B, max(max_iv, 1), 2), dtype=torch.int32, device=self.device),
                                   "audit": torch.zeros((B + 1, _lib.JOIN_AUDIT_WORDS), dtype=torch.int64, device=self.device),
                                   "ws": torch.zeros(max(need, 16), dtype=torch.uint8, device=self.device)}
            self._check(self.lib.uvad_cuts_join(self.ctx, ct["table"].data_ptr() if mc else None, ct["row_first"].data_ptr(), ct["total"].data_ptr(),
                                                mc, B, iv.data_ptr() if max_iv else None, cn.data_ptr(), max_iv, self.JOIN_MODES[mode],
                                                jn["pair_first"].data_ptr(), jn["pairs"].data_ptr() if mp else None, mp,
                                                jn["item_cuts"].data_ptr(), jn["audit"].data_ptr(), jn["ws"].data_ptr(), jn["ws"].numel(),
                                                self._stream()))
            jn["_keep"] = (iv, cn)          # the launch reads them after this call returns
            jn["max_pairs"], jn["max_iv"], jn["max_cuts"] = mp, max_iv, mc
            return {"pair_first": jn["pair_first"], "pairs": jn["pairs"][:mp], "item_cuts": jn["item_cuts"][:, :max_iv], "audit": jn["audit"]}

    def cuts_join_read(self, cuts) -> dict:
        """The last cuts_join on the state, copied to the host (synchronises) -> {"pairs_per_cut": for each cut that took part (the order of
        cuts_read) the list of its items' indices within its row, ascending; "total_pairs": the true number of pairs; "stored_pairs":
        min(total_pairs, max_pairs) -- a cut whose pairs were cut off by max_pairs lists the stored ones only --; "item_cuts" (B, max_iv,
        2) int32 {first cut, number of cuts} per item (slots past a row's count hold what an earlier call left); "audit": {"rows": one
        dict per row, "pooled": their sum} under the reference's seven names (predict.py:597-611) plus "New cuts"; "audit_words"
        (B + 1, 8) int64, the raw words}."""
        jn = cuts.get("join")
        if jn is None:
            raise RuntimeError("cuts_join_read needs a state on which cuts_join has run")
        with torch.cuda.device(self.device):
            m = min(int(cuts["total"].cpu()[0]), jn["max_cuts"])
            first = jn["pair_first"][:m + 1].cpu().numpy()
            total = int(first[m])
            stored = min(total, jn["max_pairs"])
            pairs = jn["pairs"][:stored].cpu().numpy()
            words = jn["audit"].cpu().numpy().copy()
            named = [{name: int(row[k]) for name, k in self.JOIN_AUDIT_NAMES} for row in words]
            return {"pairs_per_cut": [pairs[min(int(first[i]), stored):min(int(first[i + 1]), stored)].tolist() for i in range(m)],
                    "total_pairs": total, "stored_pairs": stored, "item_cuts": jn["item_cuts"][:, :jn["max_iv"]].cpu().numpy().copy(),
                    "audit": {"rows": named[:-1], "pooled": named[-1]}, "audit_words": words}

    # ------------------------------------------------------------------ channel fusion (uvad_fuse_*)
    FUSE_MODES = {"max": _lib.FUSE_MAX, "mean": _lib.FUSE_MEAN, "vote": _lib.FUSE_VOTE}
    FUSE_STAT_NAMES = ("valid", "speech", "agree", "best")     # the four uint64 words per member slot of d_stats, in order

    def _fuse_configure(self, st):
        """Make `st` the context's fusion configuration (one per context: the last fuse_open, or the state a call names)."""
        if getattr(self, "_fuse_current", None) is st:
            return
        first, members, w = st["first"], st["members"], st["weights"]
        self._check(self.lib.uvad_fuse_configure(self.ctx, C.byref(st["cfg"]), first.ctypes.data, members.ctypes.data,
                                                 w.ctypes.data if w is not None else None, st["G"]))
        self._fuse_current = st

    def fuse_open(self, groups, **cfg):
        """The configuration and the buffers of the fusion calls below.  groups: one list of input rows per recording (rows need not be
        contiguous and may appear in several groups); **cfg: mode "max" / "mean" / "vote", threshold, decide, weights, as
        postprocess.fuse_config, which validates them.  The configuration is uploaded into the context (uvad_fuse_configure); the
        context holds one, so a call on another state re-configures first.  Buffers are sized by the first call with a shape; after that
        the calls allocate nothing and can be captured.  st["stats"] (N, 4) int64 accumulates over calls until fuse_reset_stats."""
        from .postprocess import fuse_config
        q = fuse_config(groups=groups, **cfg)
        first = np.zeros(len(q["groups"]) + 1, np.int32)
        first[1:] = np.cumsum([len(g) for g in q["groups"]])
        members = np.ascontiguousarray(np.concatenate([np.asarray(g, np.int32) for g in q["groups"]]))
        w = None if q["weights"] is None else np.ascontiguousarray(np.concatenate([np.asarray(v, np.float32) for v in q["weights"]]))
        st = {"cfg": _lib.FuseCfg(self.FUSE_MODES[q["mode"]], float(q["threshold"]), float(q["decide"])), "config": q,
              "groups": q["groups"], "first": first, "members": members, "weights": w, "G": len(q["groups"]), "N": int(first[-1]),
              "fused": None, "glens": None, "labels": None, "best": None, "flags": None, "ws": None}
        with torch.cuda.device(self.device):
            st["stats"] = torch.zeros((st["N"], _lib.FUSE_STATS_WORDS), dtype=torch.int64, device=self.device)
            self._fuse_configure(st)
        return st

    def fuse_reset_stats(self, state):
        state["stats"].zero_()

    def _fuse_buffers(self, st, T: int, labels: bool, best: bool, flags: bool):
        G = st["G"]
        if st["fused"] is None or tuple(st["fused"].shape) != (G, T):
            st["fused"] = torch.zeros((G, T), dtype=torch.float32, device=self.device)
            st["glens"] = torch.zeros(G, dtype=torch.int32, device=self.device)
            st["labels"] = st["best"] = None
        if labels and st["labels"] is None:
            st["labels"] = torch.zeros((G, T), dtype=torch.uint8, device=self.device)
        if best and st["best"] is None:
            st["best"] = torch.zeros((G, T), dtype=torch.uint8, device=self.device)
        if flags and st["flags"] is None:
            st["flags"] = torch.zeros(G, dtype=torch.uint8, device=self.device)

    def _fuse_enqueue(self, st, in_ptr, ld_in, B, T, lens_ptr, flags_ptr, labels: bool, best: bool, stats: bool = True):
        return self.lib.uvad_fuse(self.ctx, in_ptr, ld_in, B, T, lens_ptr, flags_ptr, st["fused"].data_ptr(), st["fused"].shape[1],
                                  st["glens"].data_ptr(), st["flags"].data_ptr() if flags_ptr is not None else None,
                                  st["labels"].data_ptr() if labels else None, T, st["best"].data_ptr() if best else None, T,
                                  st["stats"].data_ptr() if stats else None, st["ws"].data_ptr(), st["ws"].numel(), self._stream())

    def fuse(self, probs: "torch.Tensor", lengths=None, state=None, labels: bool = True, best: bool = True, **cfg):
        """probs (B, T) f32 on the GPU, one row per channel (row-strided views are used as they are; logits do as well), lengths (B,)
        valid frames per row (a device tensor is read on the device).  state: one of fuse_open; without it one is opened from **cfg
        (groups=...).  -> (fused (G, T) f32, glens (G,) int32, labels (G, T) uint8 or None, best (G, T) uint8 or None, stats (N, 4) int64
        {valid, speech, agree, best} per member slot, accumulated over the calls on the state), on the device and overwritten by the next
        call on the state.  Columns at or past a group's length keep what they held (zero in a fresh state).  fuse_read gives the stats
        on the host."""
        st = state if state is not None else self.fuse_open(**cfg)
        with torch.cuda.device(self.device):
            if not torch.is_tensor(probs) or probs.device != self.device:
                raise RuntimeError(f"probs must be a tensor on {self.device}")
            probs = self._rows_2d(probs, torch.float32, "probs")
            B, T = probs.shape
            if B <= int(st["members"].max()):
                raise ValueError(f"probs has {B} rows, the groups name row {int(st['members'].max())}")
            n = None if lengths is None else self._dev_lens(lengths, B, T, torch.int32, "lengths (frames)")
            self._fuse_configure(st)
            self._fuse_buffers(st, T, labels, best, False)
            need = int(self.lib.uvad_fuse_ws_bytes(self.ctx, B, T))
            if st["ws"] is None or st["ws"].numel() < need:
                st["ws"] = torch.zeros(max(need, 16), dtype=torch.uint8, device=self.device)
            self._check(self._fuse_enqueue(st, probs.data_ptr(), probs.stride(0) if B > 1 else max(probs.stride(0), T), B, T,
                                           n.data_ptr() if n is not None else None, None, labels, best))
            st["_keep"] = (probs, n)   # the launch reads them after this call returns
            return st["fused"], st["glens"], st["labels"] if labels else None, st["best"] if best else None, st["stats"]

    def fuse_pick(self, best: "torch.Tensor", cuts, state=None):
        """The channel of each cut (uvad_fuse_pick): best (G, T) uint8 as fuse wrote it, cuts a state of cuts_open on which cuts_table
        has run on the fused labels.  -> (table (max_cuts, 8) int32, the cut table with each row replaced by the picked member's input
        row -- pass it to cuts_gather(..., table=) with the (B, S) audio rows --, picks (max_cuts,) int32, the position within the
        group; -1 for a cut whose row is no group), on the device, kept on the state and overwritten by the next call."""
        ct = cuts
        if ct.get("table") is None:
            raise RuntimeError("fuse_pick needs a state on which cuts_table has run")
        with torch.cuda.device(self.device):
            if not torch.is_tensor(best) or best.device != self.device:
                raise RuntimeError(f"best must be a tensor on {self.device}")
            best = self._rows_2d(best, torch.uint8, "best")
            if state is not None:
                self._fuse_configure(state)
            mc = ct["max_cuts"]
            if ct.get("pick_table") is None or ct["pick_table"].shape[0] != max(mc, 1):
                ct["pick_table"] = torch.zeros((max(mc, 1), 8), dtype=torch.int32, device=self.device)
                ct["pick"] = torch.zeros(max(mc, 1), dtype=torch.int32, device=self.device)
            self._check(self.lib.uvad_fuse_pick(self.ctx, best.data_ptr(), best.stride(0) if best.shape[0] > 1 else max(best.stride(0), best.shape[1]),
                                                ct["table"].data_ptr() if mc else None, ct["total"].data_ptr(), mc,
                                                ct["pick_table"].data_ptr(), ct["pick"].data_ptr(), self._stream()))
            ct["_keep_best"] = best
            return ct["pick_table"][:mc], ct["pick"][:mc]

    def fuse_read(self, state):
        """The counters accumulated on the state, copied to the host (synchronises): per group a list with one dict {valid, speech,
        agree, best} per member, in slot order."""
        with torch.cuda.device(self.device):
            words = state["stats"].cpu().numpy()
        first = state["first"]
        return [[{name: int(words[j, k]) for k, name in enumerate(self.FUSE_STAT_NAMES)} for j in range(first[g], first[g + 1])]
                for g in range(state["G"])]

    # ------------------------------------------------------------------ hysteresis decisions with minimum durations (uvad_binarize)
    def binarize_open(self, onset: float = 0.5, offset=None, min_on: int = 0, min_off: int = 0, pad_on: int = 0, pad_off: int = 0, max_iv=None):
        """The configuration and the buffers of binarize below: speech turns on at a frame with !(p < onset) and off at one with p < offset
        (default: onset), every run is widened by pad_on frames before and pad_off after, pauses shorter than min_off frames are filled and
        intervals shorter than min_on frames dropped, in that order (postprocess.binarize_config makes these from seconds).  max_iv: the
        intervals stored per row (default (T + 1) // 2, which never overflows).  Buffers are sized by the first call with a shape; after
        that the call allocates nothing and can be captured."""
        offset = onset if offset is None else offset
        ints = {"min_on": min_on, "min_off": min_off, "pad_on": pad_on, "pad_off": pad_off}
        ok = all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) and 0 <= int(v) <= (1 << 20) for v in ints.values())
        if not ok or not (np.isfinite(onset) and np.isfinite(offset)) or float(np.float32(offset)) > float(np.float32(onset)):
            raise ValueError(f"bad binarize configuration: onset {onset} and offset {offset} must be finite with offset <= onset; "
                             f"min_on {min_on}, min_off {min_off}, pad_on {pad_on} and pad_off {pad_off} must be integers in 0 .. 2^20 frames")
        if max_iv is not None and int(max_iv) < 0:
            raise ValueError("max_iv must be >= 0")
        cfg = _lib.BinarizeCfg(float(onset), float(offset), int(min_on), int(min_off), int(pad_on), int(pad_off))
        return {"cfg": cfg, "max_iv": None if max_iv is None else int(max_iv), "labels": None, "iv": None, "counts": None, "ws": None}

    def binarize(self, probs: "torch.Tensor", lengths=None, state=None, labels: bool = True, **cfg):
        """probs (B, T) f32 on the GPU (row-strided views are used as they are), lengths (B,) valid frames per row (a device tensor is read
        on the device).  state: one of binarize_open; without it one is opened from **cfg.  -> (labels (B, T) uint8 or None, intervals
        (B, max_iv, 2) int32 {lo, hi}, counts (B,) int32 -- the true numbers, which may exceed max_iv), on the device and overwritten by
        the next call on the state.  Label columns at or past a row's length keep what they held (zero in a fresh state).  binarize_read
        gives the host view."""
        st = state if state is not None else self.binarize_open(**cfg)
        with torch.cuda.device(self.device):
            if not torch.is_tensor(probs) or probs.device != self.device:
                raise RuntimeError(f"probs must be a tensor on {self.device}")
            probs = self._rows_2d(probs, torch.float32, "probs")
            B, T = probs.shape
            n = None if lengths is None else self._dev_lens(lengths, B, T, torch.int32, "lengths (frames)")
            if st["max_iv"] is None:
                st["max_iv"] = (T + 1) // 2
            mi = st["max_iv"]
            if st["iv"] is None or st["iv"].shape[0] != B:
                st["iv"] = torch.zeros((B, max(mi, 1), 2), dtype=torch.int32, device=self.device)
                st["counts"] = torch.zeros(B, dtype=torch.int32, device=self.device)
            if labels and (st["labels"] is None or tuple(st["labels"].shape) != (B, T)):
                st["labels"] = torch.zeros((B, T), dtype=torch.uint8, device=self.device)
            need = int(self.lib.uvad_binarize_ws_bytes(self.ctx, B, T))
            if st["ws"] is None or st["ws"].numel() < need:
                st["ws"] = torch.zeros(max(need, 16), dtype=torch.uint8, device=self.device)
            lab = st["labels"] if labels else None
            self._check(self.lib.uvad_binarize(self.ctx, probs.data_ptr(), probs.stride(0) if B > 1 else max(probs.stride(0), T), B, T,
                                               n.data_ptr() if n is not None else None, C.byref(st["cfg"]),
                                               lab.data_ptr() if lab is not None else None, T, st["iv"].data_ptr() if mi else None, mi,
                                               st["counts"].data_ptr(), st["ws"].data_ptr(), st["ws"].numel(), self._stream()))
            st["_keep"] = (probs, n)   # the launch reads them after this call returns
            return lab, st["iv"][:, :mi], st["counts"]

    def binarize_read(self, state):
        """The intervals the last binarize on the state listed, copied to the host (synchronises): per row [(lo, hi)] in frames, the
        first min(count, max_iv) of each row."""
        if state.get("iv") is None:
            raise RuntimeError("binarize_read needs a state on which binarize has run")
        with torch.cuda.device(self.device):
            cn = state["counts"].cpu().numpy()
            iv = state["iv"].cpu().numpy()
        return [[(int(lo), int(hi)) for lo, hi in iv[b, :min(int(cn[b]), state["max_iv"])]] for b in range(len(cn))]

    # ------------------------------------------------------------------ sliding windows over whole recordings (uvad_sliding_*)
    def sliding_configure(self, window: int, hop: int, weights=None):
        """Window and hop in frames and the aggregation weights (W,) -- None: all ones; postprocess.sliding_weights makes the usual ones
        -- of the sliding calls below (uvad_sliding_configure).  The table is uploaded here, once."""
        w = None
        if weights is not None:
            w = np.ascontiguousarray(np.asarray(weights.detach().cpu() if torch.is_tensor(weights) else weights), np.float32)
            if w.shape != (int(window),):
                raise ValueError(f"weights must have shape ({int(window)},), got {w.shape}")
        with torch.cuda.device(self.device):
            self._check(self.lib.uvad_sliding_configure(self.ctx, int(window), int(hop), w.ctypes.data if w is not None else None))
        self._sliding = (int(window), int(hop))

    def _sliding_call(self, fn, ws_bytes, x, R, L, T, n, host_frames, first, group, tap):
        """ws_bytes(N, group) -> workspace size; L: the row length the entry point takes (frames or samples), T: frames per output row."""
        if getattr(self, "_sliding", None) is None:
            raise RuntimeError("call sliding_configure(window, hop, weights) first")
        W, Hf = self._sliding
        if first is None:
            first = sliding_plan(host_frames, W, Hf)[1]
        first = [int(v) for v in first]
        if len(first) != R + 1:
            raise ValueError(f"first must hold {R + 1} prefix sums, got {len(first)}")
        N = first[-1]
        group = max(1, min(int(group), max(N, 1)))
        d_first = torch.tensor(first, dtype=torch.int32, device=self.device)
        need = int(ws_bytes(N, group))
        if self._ws is None or self._ws.numel() < need:
            self._ws = None
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        probs = torch.empty((R, T), dtype=torch.float32, device=self.device)
        frames = torch.empty(R, dtype=torch.int32, device=self.device)
        win = torch.empty((N, W), dtype=torch.float32, device=self.device) if tap else None
        self._check(fn(self.ctx, x.data_ptr(), R, L, n.data_ptr(), d_first.data_ptr(), N, group, probs.data_ptr(), T, frames.data_ptr(),
                       win.data_ptr() if tap and N else None, self._ws.data_ptr(), self._ws.numel(), self._stream()))
        return (probs, frames, win) if tap else (probs, frames)

    @staticmethod
    def _host_lengths(lengths):
        return [int(v) for v in (lengths.tolist() if torch.is_tensor(lengths) else lengths)]

    def sliding_classify(self, feats: "torch.Tensor", lengths, group: int = 512, first=None, tap: bool = False):
        """feats (R,T,F) on the GPU, lengths: valid frames per recording (R,) -> (probs (R,T), frames int32 (R,)): every recording
        covered by windows of the configured length and hop (sliding_plan), each run from zero state on its own length, a frame's
        probability the weighted mean over the windows that cover it; 0 past a recording's length (uvad_sliding_classify).  group: windows
        per classifier launch (bounds the workspace, not the result).  first: another window list than sliding_plan's (R + 1 prefix
        sums).  tap: also return every window's probabilities (N, W)."""
        with torch.cuda.device(self.device):
            feats = self._dev_f32(feats, "feats")
            R, T, F = feats.shape
            if F != self._mc_c.in_dim:
                raise ValueError(f"feature dim {F} != encoding_dim {self._mc_c.in_dim}")
            host = [min(max(v, 0), T) for v in self._host_lengths(lengths)]
            n = self._dev_lens(lengths, R, T, torch.int32, "lengths (frames)")
            ws = lambda N, g: self.lib.uvad_sliding_workspace_bytes(self.ctx, R, T, N, g)   # noqa: E731
            return self._sliding_call(self.lib.uvad_sliding_classify, ws, feats, R, T, T, n, host, first, group, tap)

    def sliding_forward(self, pcm: "torch.Tensor", lengths, group: int = 512, first=None, tap: bool = False):
        """pcm (R,S) f32 or int16 on the GPU, lengths: samples per recording (R,) -> (probs (R,T), frames (R,)), T = num_frames(S): the
        recordings' continuous log-mel rows are computed once (uvad_fbank_lens), then as sliding_classify (uvad_sliding_forward[_i16])."""
        with torch.cuda.device(self.device):
            pcm, i16 = self._dev_wav(pcm)
            R, S = pcm.shape
            T = self.num_frames(S)
            if T <= 0:
                raise ValueError(f"{S} samples are too short for one frame")
            host = [self.num_frames(min(max(v, 0), S)) for v in self._host_lengths(lengths)]
            n = self._dev_lens(lengths, R, S, torch.int64, "lengths (samples)")
            fn = self.lib.uvad_sliding_forward_i16 if i16 else self.lib.uvad_sliding_forward
            ws = lambda N, g: self.lib.uvad_sliding_workspace_bytes(self.ctx, R, T, N, g)   # noqa: E731
            return self._sliding_call(fn, ws, pcm, R, S, T, n, host, first, group, tap)

    def sliding_forward_wav(self, wav: "torch.Tensor", lengths, group: int = 512, first=None, tap: bool = False):
        """The waveform model: wav (R,S) f32 or int16, lengths: samples per recording -> (probs (R,T), frames (R,)), T =
        sincnet_num_frames(S).  Window j of a recording is its samples from 270 * hop * j on (991 + 270 * (W - 1) of them, clipped to the
        recording), through SincNet with every norm over the window's own samples (uvad_sliding_forward_wav[_i16])."""
        if self._sn_c is None:
            raise RuntimeError("this runtime was created without a SincNet configuration")
        with torch.cuda.device(self.device):
            wav, i16 = self._dev_wav(wav)
            R, S = wav.shape
            T = self.sincnet_num_frames(S)
            if T <= 0:
                raise ValueError(f"{S} samples are too short for one SincNet frame")
            host = [self.sincnet_num_frames(min(max(v, 0), S)) for v in self._host_lengths(lengths)]
            n = self._dev_lens(lengths, R, S, torch.int64, "lengths (samples)")
            fn = self.lib.uvad_sliding_forward_wav_i16 if i16 else self.lib.uvad_sliding_forward_wav
            ws = lambda N, g: self.lib.uvad_sliding_wav_workspace_bytes(self.ctx, R, S, N, g)   # noqa: E731
            return self._sliding_call(fn, ws, wav, R, S, T, n, host, first, group, tap)

    # ------------------------------------------------------------------ ingest stage: audio as it arrives -> (rows, samples) f32 at 16 kHz
    _INGEST_DTYPES = {"f32": torch.float32, "int16": torch.int16, "ulaw": torch.uint8, "alaw": torch.uint8}

    def ingest_configure(self, encoding: str, channels: int = 1, sample_rate: int = 16000, taps=None):
        """Describe the source of ingest() / ingest_step() (uvad_ingest_configure): encoding "f32", "int16" (q / 32768), "ulaw" or "alaw"
        (G.711 bytes); `channels` interleaved channels, each of which becomes an output row of its own (row b * channels + c, no
        down-mix); sample_rate in Hz.  taps: a polyphase table (up, 2 * width + down) for 16000 / sample_rate = up / down; default
        resample_taps(sample_rate), the published Hann-windowed sinc design.  16 kHz takes no table.  Returns ingest_plan's geometry."""
        if encoding not in ENCODINGS:
            raise ValueError(f"encoding must be one of {sorted(ENCODINGS)}, got {encoding!r}")
        up, down = resample_ratio(sample_rate)
        width = 0
        if (up, down) != (1, 1):
            if taps is None:
                taps, up, down, width = resample_taps(sample_rate)
            else:
                taps = np.ascontiguousarray(taps, np.float32)
                if taps.ndim != 2 or taps.shape[0] != up or taps.shape[1] < down or (taps.shape[1] - down) % 2:
                    raise ValueError(f"taps must have shape ({up}, 2 * width + {down}), got {taps.shape}")
                width = (taps.shape[1] - down) // 2
        cfg = _lib.IngestCfg(ENCODINGS[encoding], int(channels), int(sample_rate))
        self._check(self.lib.uvad_ingest_configure(self.ctx, C.byref(cfg)))
        self._ingest = None
        if (up, down) != (1, 1):
            self._check(self.lib.uvad_ingest_set_taps(self.ctx, taps.ctypes.data, up, down, width))
        D, H = stream_delay(up, down, width)
        self._ingest = {"encoding": encoding, "dtype": self._INGEST_DTYPES[encoding], "channels": int(channels), "sample_rate": int(sample_rate),
                        "up": up, "down": down, "width": width, "delay": D, "history": H}
        return dict(self._ingest)

    def _ingest_input(self, x, frames=None, contiguous=True):
        ig = getattr(self, "_ingest", None)
        if ig is None:
            raise RuntimeError("call ingest_configure first")
        if not torch.is_tensor(x) or x.device != self.device or x.dtype != ig["dtype"]:
            raise RuntimeError(f"the {ig['encoding']} source must be a {ig['dtype']} tensor on {self.device}")
        Cn = ig["channels"]
        if x.dim() == 2 and Cn == 1:
            x = x.unsqueeze(-1)
        if x.dim() != 3 or x.shape[2] != Cn or (frames is not None and x.shape[1] != frames):
            raise ValueError(f"expected (rows, {'frames' if frames is None else frames}, {Cn}) interleaved input, got {tuple(x.shape)}")
        return ig, (x.contiguous() if contiguous else x)

    def ingest(self, x: "torch.Tensor", lengths=None, out=None):
        """x (B, S_in, channels) -- (B, S_in) for one channel -- in the configured encoding on the GPU -> (B * channels, ceil(up * S_in /
        down)) f32 at 16 kHz, row b * channels + c (uvad_ingest).  lengths: input frames per row (B,): row b is ingested as x[b, :lengths[b]]
        alone, what lies past it is never read and the output past its count is +0; returns (out, counts int64 (B * channels,)) with the
        per-row output counts on the device, as forward(..., lengths=) / forward_wav(..., lengths=) take them (uvad_ingest_lens).
        out: a contiguous f32 tensor of the output's shape on this device to write into (a caller that ingests the same shape again and
        again keeps one), else a new one."""
        with torch.cuda.device(self.device):
            ig, x = self._ingest_input(x)
            B, S_in, Cn = x.shape
            S_out = -(-(ig["up"] * S_in) // ig["down"])
            if out is None:
                out = torch.empty((B * Cn, S_out), dtype=torch.float32, device=self.device)
            elif (not torch.is_tensor(out) or out.device != self.device or out.dtype != torch.float32 or tuple(out.shape) != (B * Cn, S_out)
                  or not out.is_contiguous()):
                raise ValueError(f"out must be a contiguous float32 tensor of shape ({B * Cn}, {S_out}) on {self.device}")
            if lengths is None:
                if B and S_in:
                    self._check(self.lib.uvad_ingest(self.ctx, x.data_ptr(), B, S_in, out.data_ptr(), self._stream()))
                return out
            n = self._dev_lens(lengths, B, S_in, torch.int64, "lengths (input frames)")
            counts = torch.empty(B * Cn, dtype=torch.int64, device=self.device)
            src = x if x.numel() else torch.zeros(1, dtype=x.dtype, device=self.device)   # (a non-null pointer that is never read)
            self._check(self.lib.uvad_ingest_lens(self.ctx, src.data_ptr(), B, S_in, n.data_ptr(), out.data_ptr() if S_out else None,
                                                  counts.data_ptr(), self._stream()))
            return out, counts

    def ingest_open(self, B: int, chunk_in: int, graphs: bool = False):
        """Allocate and reset an ingest stream (uvad_ingest_stream_reset): B feeds x channels in lockstep, chunk_in input frames per step
        (a multiple of `down`).  Its output is the dense ingest delayed by the plan's `delay` samples: the first `delay` samples of a
        session are +0, the last `delay` are never produced.  graphs: capture the first step into a hipGraph and replay it for every
        later one (a step depends on nothing on the host)."""
        ig = getattr(self, "_ingest", None)
        if ig is None:
            raise RuntimeError("call ingest_configure first")
        if chunk_in <= 0 or chunk_in % ig["down"]:
            raise ValueError(f"chunk_in must be a positive multiple of down = {ig['down']}, got {chunk_in}")
        with torch.cuda.device(self.device):
            nbytes = int(self.lib.uvad_ingest_state_bytes(self.ctx, B))
            if nbytes == 0:
                raise RuntimeError("ingest streams need ingest_configure (and a table where the rate needs one)")
            state = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            self._check(self.lib.uvad_ingest_stream_reset(self.ctx, state.data_ptr(), nbytes, B, self._stream()))
            rows = B * ig["channels"]
            return {"state": state, "B": B, "chunk_in": chunk_in, "rows": rows, "delay": ig["delay"],
                    "out": torch.empty((rows, chunk_in // ig["down"] * ig["up"]), dtype=torch.float32, device=self.device),
                    "in": torch.empty((B, chunk_in, ig["channels"]), dtype=ig["dtype"], device=self.device),
                    "flags": torch.zeros(rows, dtype=torch.uint8, device=self.device), "flags_set": False,
                    "graphs": 0 if graphs else None, "graph": None}

    def ingest_step(self, st, chunk: "torch.Tensor", start=None) -> "torch.Tensor":
        """chunk (B, chunk_in, channels) in the configured encoding on the GPU -> (B * channels, chunk_in * up / down) f32, a buffer the
        next step overwrites; hand it to any *_stream_step / *_slots_step.  start: output rows (a bool mask of B * channels entries or
        an index list, as the slot pools' `start`) whose session begins with this chunk: their history is zeroed first."""
        with torch.cuda.device(self.device):
            _, chunk = self._ingest_input(chunk, st["chunk_in"], contiguous=st["graphs"] is None)   # (the graph's fixed buffer takes any strides)
            if chunk.shape[0] != st["B"]:
                raise ValueError(f"expected {st['B']} rows, got {chunk.shape[0]}")
            out = st["out"]

            def enqueue(src, flags):
                return self.lib.uvad_ingest_stream_step(self.ctx, src.data_ptr(), flags.data_ptr() if flags is not None else None, st["B"],
                                                        st["chunk_in"], st["state"].data_ptr(), st["state"].numel(), out.data_ptr(),
                                                        self._stream())

            if st["graphs"] is None:
                self._check(enqueue(chunk, self._slot_flags(st["rows"], start, None)))
                return out
            st["in"].copy_(chunk)
            if start is not None:
                self._slot_flags(st["rows"], start, None, st["flags"])
                st["flags_set"] = True
            elif st["flags_set"]:                            # (a step without starts costs no flag kernels once the buffer is clear)
                st["flags"].zero_()
                st["flags_set"] = False
            if st["graph"] is None:
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):                    # capture: recorded, not run
                    r = enqueue(st["in"], st["flags"])
                self._check(r)
                st["graph"] = g
                st["graphs"] += 1
            st["graph"].replay()
            return out

    def set_gemm_mode(self, mode: str):
        """"f32": exact f32 MFMA; "f16p": split-f16 on the f16 matrix cores (default: the weight-stationary kernel for the large
        projections, the tile-streaming one elsewhere); "f16p_stream": split-f16 with the tile-streaming kernel only (same bits,
        kept for A/B runs and as the reference of the bit-identity test); "f16p3": "f16p" with three instead of four MFMA products
        per f32-equivalent product in the large-launch kernels (weights rounded to 22 bits; faster, see include/uvad.h)."""
        self._check(self.lib.uvad_set_gemm_mode(self.ctx, {"f32": 0, "f16p": 1, "f16p_stream": 2, "f16p3": 3}[mode]))

    def set_recurrent_tile(self, sequences: int):
        """Sequences per recurrent workgroup: 0 (default) = chosen from the batch size, 4 = latency form, 16 = throughput form."""
        self._check(self.lib.uvad_set_recurrent_tile(self.ctx, int(sequences)))

    def recurrent_tile_for(self, batch: int) -> int:
        """What the default choice would launch for `batch` sequences (4 or 16)."""
        return int(self.lib.uvad_recurrent_tile_for(self.ctx, int(batch)))

    def recurrent_tile(self) -> int:
        """What the most recent classify / forward launched (4 or 16)."""
        return int(self.lib.uvad_get_recurrent_tile(self.ctx))

    def p2_on_fp8(self) -> bool:
        """True if the 16-sequence recurrence runs its P2 x h product on the 8-bit matrix pipe (every P2 element exactly bf8: include/uvad.h)."""
        return bool(self.lib.uvad_get_p2_on_fp8(self.ctx))

    def weights_shared_by(self) -> int:
        """How many contexts of this process use this context's packed weights on the device (include/uvad.h: contexts finalized with
        identical tensors share them; 1 = not shared)."""
        return int(self.lib.uvad_weights_shared_by(self.ctx))

    def sincnet_form(self) -> str:
        """What the most recent sincnet() / forward_wav() ran: "f16p" (the split-f16 stages of sincnet_f16p.hip) or "f32" (sincnet.hip)."""
        return "f16p" if int(self.lib.uvad_get_sincnet_form(self.ctx)) == 1 else "f32"

    def set_time_chunks(self, chunks: int):
        """Time chunks per layer for a batch that runs alone (include/uvad.h): 0 = automatic (default), 1 = off, n = that many.  The
        projection of chunk i + 1 runs on a stream of the library's own beside the recurrence of chunk i; outputs are bit-identical."""
        self._check(self.lib.uvad_set_time_chunks(self.ctx, int(chunks)))

    def time_chunks(self) -> int:
        """What the most recent classify / forward ran (1 = not chunked)."""
        return int(self.lib.uvad_get_time_chunks(self.ctx))

    def set_concurrent_steps(self, n: int):
        """Steps the caller keeps in flight at once, this context's included (include/uvad.h): with n > 1 the persistent projection
        and head grids leave the other steps' recurrences their CUs.  1 = the call runs alone (default); outputs are bit-identical."""
        self._check(self.lib.uvad_set_concurrent_steps(self.ctx, int(n)))

    def concurrent_steps(self) -> int:
        return int(self.lib.uvad_get_concurrent_steps(self.ctx))

    def projection_grid(self) -> int:
        """Workgroups of the weight-stationary projection launches of the most recent classify / forward (0 = it launched none)."""
        return int(self.lib.uvad_get_projection_grid(self.ctx))

    def der_counts(self, pred: "torch.Tensor", gt: "torch.Tensor") -> "torch.Tensor":
        """pred, gt (B, T) uint8 0/1 on the GPU -> (B, 2) int32 counts {false alarm, missed detection}."""
        with torch.cuda.device(self.device):
            pred = pred.to(torch.uint8).contiguous()
            gt = gt.to(self.device, torch.uint8).contiguous()
            B, T = pred.shape
            out = torch.empty((B, 2), dtype=torch.int32, device=self.device)
            self._check(self.lib.uvad_der_counts(self.ctx, pred.data_ptr(), gt.data_ptr(), B, T, out.data_ptr(), self._stream()))
            return out

    def label_runs(self, labels: "torch.Tensor", max_runs: int = 0, lengths=None):
        """labels (B, T) uint8 0/1 on the GPU -> (runs (B, max_runs, 2) int32, counts (B,) int32), both on the GPU.
        lengths: valid frames per row (B,): runs of each row's prefix, a run open at its end closes at lengths[b]."""
        with torch.cuda.device(self.device):
            if not torch.is_tensor(labels) or labels.device != self.device:
                raise RuntimeError(f"labels must be a tensor on {self.device}")
            labels = labels.to(torch.uint8).contiguous()
            B, T = labels.shape
            max_runs = int(max_runs) if max_runs > 0 else (T + 1) // 2
            runs = torch.empty((B, max_runs, 2), dtype=torch.int32, device=self.device)
            counts = torch.empty((B,), dtype=torch.int32, device=self.device)
            if lengths is None:
                self._check(self.lib.uvad_label_runs(self.ctx, labels.data_ptr(), B, T, max_runs, runs.data_ptr(), counts.data_ptr(), self._stream()))
            else:
                n = self._dev_lens(lengths, B, T, torch.int32, "lengths (frames)")
                self._check(self.lib.uvad_label_runs_lens(self.ctx, labels.data_ptr(), B, T, n.data_ptr(), max_runs, runs.data_ptr(),
                                                          counts.data_ptr(), self._stream()))
            return runs, counts

    def streams_overlap(self, a: "torch.cuda.Stream", b: "torch.cuda.Stream") -> bool:
        """True if kernels on the two HIP streams run concurrently (they sit on different hardware queues)."""
        r = self.lib.uvad_streams_overlap(self.ctx, C.c_void_p(a.cuda_stream), C.c_void_p(b.cuda_stream))
        if r < 0:
            self._check(r)
        return r == 1

    def set_timing(self, on: bool):
        self._check(self.lib.uvad_set_timing(self.ctx, int(on)))

    def timing_ms(self):
        buf = (C.c_float * 5)()
        self._check(self.lib.uvad_get_timing(self.ctx, buf))
        return dict(zip(("fbank", "proj", "recurrent", "head", "total"), [float(x) for x in buf]))

    def layer_timing_ms(self):
        """[(projection ms, recurrence ms)] per LSTM layer of the last timed call."""
        n = 2 * self._mc_c.num_layers
        buf = (C.c_float * n)()
        got = self.lib.uvad_get_layer_timing(self.ctx, buf, n)
        if got < 0:
            self._check(got)
        return [(float(buf[2 * k]), float(buf[2 * k + 1])) for k in range(got // 2)]

    # ------------------------------------------------------------------ teardown
    def close(self):
        self._drop_lstm_prefix()
        if getattr(self, "ctx", None) is not None and self.ctx:
            self.lib.uvad_destroy(self.ctx)
            self.ctx = C.c_void_p()
        self._ws = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
