"""ctypes binding of libuvad.so (include/uvad.h).  No torch types cross this boundary: only raw
device pointers, sizes and a hipStream_t.  There is no CPU fallback: if the shared object is
missing, ``load()`` raises with the build command instead of degrading to a torch path."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libuvad.so")

UVAD_OK = 0
ERR_NAMES = {-1: "UVAD_E_ARG", -2: "UVAD_E_HIP", -3: "UVAD_E_STATE", -4: "UVAD_E_WORKSPACE", -5: "UVAD_E_UNSUPPORTED"}
ABI_VERSION = 5
SLOT_START, SLOT_END = 1, 2      # the flag bits of a slot pool step (uvad_window_slots_step, include/uvad.h)


class FbankCfg(C.Structure):
    _fields_ = [("sample_rate", C.c_int), ("frame_len", C.c_int), ("frame_shift", C.c_int),
                ("n_fft", C.c_int), ("n_mels", C.c_int),
                ("preemph", C.c_float), ("low_hz", C.c_float), ("high_hz", C.c_float),
                ("log_floor", C.c_float), ("remove_dc", C.c_int), ("snip_edges", C.c_int)]


class ModelCfg(C.Structure):
    _fields_ = [("in_dim", C.c_int), ("hidden", C.c_int), ("num_layers", C.c_int),
                ("bidirectional", C.c_int), ("lin_hidden", C.c_int), ("lin_layers", C.c_int),
                ("leaky_slope", C.c_float)]


class SincNetCfg(C.Structure):
    _fields_ = [("stride", C.c_int), ("n_filters", C.c_int), ("kernel_size", C.c_int), ("c2", C.c_int), ("k2", C.c_int),
                ("c3", C.c_int), ("k3", C.c_int), ("leaky_slope", C.c_float), ("eps", C.c_float)]


class IngestCfg(C.Structure):
    _fields_ = [("encoding", C.c_int), ("channels", C.c_int), ("sample_rate", C.c_int)]


class EndpointCfg(C.Structure):
    _fields_ = [("kernel", C.c_int), ("pad", C.c_int), ("threshold", C.c_float)]


SCORE_MAX_POINTS = 8
SCORE_TOTALS_WORDS = 2088        # uint64 words uvad_score_totals writes (include/uvad.h gives the layout)


class ScoreCfg(C.Structure):
    _fields_ = [("n_points", C.c_int), ("threshold", C.c_float * SCORE_MAX_POINTS), ("kernel", C.c_int * SCORE_MAX_POINTS),
                ("collar", C.c_int), ("bins", C.c_int), ("segment", C.c_int)]


CUTS_SAMPLES, CUTS_FRAMES = 0, 1     # `which` of uvad_cuts_gather


HEAD_TRAIN_MASTERS, HEAD_TRAIN_GRAD, HEAD_TRAIN_M, HEAD_TRAIN_V, HEAD_TRAIN_SCALARS = range(5)   # `which` of uvad_head_train_read
HEAD_TRAIN_SCALAR_WORDS = 8      # 32-bit words of the scalar record (include/uvad.h gives the layout)


class HeadTrainCfg(C.Structure):     # uvad_head_train_cfg (20 bytes)
    _fields_ = [("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float), ("segment", C.c_int)]


class LstmTrainCfg(C.Structure):     # uvad_lstm_train_cfg (24 bytes)
    _fields_ = [("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float), ("segment", C.c_int), ("first_layer", C.c_int)]


class SincNetTrainCfg(C.Structure):  # uvad_sincnet_train_cfg (24 bytes)
    _fields_ = [("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float), ("segment", C.c_int), ("first_stage", C.c_int)]


SINCNET_TRAIN_FILTERS = 5        # `which` of uvad_sincnet_train_read: the bank of the last forward call


LSTM_TRAIN_SCALAR_WORDS = 10     # an LSTM state's scalar record: the head's eight words, then the dropout draw ordinal (uint64)
OPTIM_RECORD_WORDS = 8           # 32-bit words of uvad_optim_read's record: norm, coef, lr_t, took-part bits, t (u64), skipped (u64)


class OptimCfg(C.Structure):     # uvad_optim_cfg (40 bytes)
    _fields_ = [("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float), ("max_norm", C.c_float), ("weight_decay", C.c_float),
                ("decoupled", C.c_int), ("skip_nonfinite", C.c_int), ("lr_scale", C.c_float * 3)]


INGEST_F32, INGEST_I16 = 0, 1    # `fmt` of uvad_mix_step / uvad_mix_apply and uvad_reverb_step / uvad_reverb_apply (UVAD_INGEST_*)
MIX_MAX_SEG, MIX_PLAN_HEAD, MIX_SEG_WORDS = 64, 4, 4     # the plan record of uvad_mix_step: int32 words per row = head + seg words x max_seg


class MixCfg(C.Structure):       # uvad_mix_cfg (32 bytes)
    _fields_ = [("mix_prob", C.c_float), ("snr_steps", C.c_int), ("h_amp", C.POINTER(C.c_double)), ("max_seg", C.c_int), ("seed", C.c_uint64)]


REVERB_PLAN_WORDS, REVERB_MAX_TAPS = 4, 1 << 20          # the plan record of uvad_reverb_step: {applied, r, d, gain bits}; taps per response at most
REVERB_TILE, REVERB_K_CHUNK = 4096, 256                  # the convolution kernel's tile constants (UVAD_REVERB_TILE, UVAD_REVERB_K_CHUNK)


class ReverbCfg(C.Structure):    # uvad_reverb_cfg (24 bytes)
    _fields_ = [("prob", C.c_float), ("normalize", C.c_int), ("align", C.c_int), ("max_taps", C.c_int), ("seed", C.c_uint64)]


SAMPLER_FBANK, SAMPLER_SINCNET = 0, 1                     # uvad_sampler_cfg.geometry (UVAD_SAMPLER_*)
SAMPLER_PLAN_WORDS, SAMPLER_MAX_SETS = 8, 64              # the plan record of uvad_sampler_step: {dataset, epoch, position, window, recording, start, n, T_b}


class SamplerCfg(C.Structure):   # uvad_sampler_cfg (56 bytes)
    _fields_ = [("window", C.c_int64), ("min_keep", C.c_int64), ("geometry", C.c_int), ("half", C.c_int), ("step", C.c_int), ("shuffle", C.c_int),
                ("drop_last", C.c_int), ("pad", C.c_int), ("batch", C.c_int), ("seed", C.c_uint64)]


class CutsCfg(C.Structure):
    _fields_ = [("pad", C.c_int), ("max_len", C.c_int), ("min_len", C.c_int), ("hop", C.c_int), ("lead", C.c_int), ("tail", C.c_int)]


JOIN_OVERLAP, JOIN_INSIDE = 0, 1     # `mode` of uvad_cuts_join
JOIN_AUDIT_WORDS = 8                 # uint64 words per row of uvad_cuts_join's d_audit (include/uvad.h gives the layout)


FUSE_MAX, FUSE_MEAN, FUSE_VOTE = 0, 1, 2     # uvad_fuse_cfg.mode
FUSE_MAX_MEMBERS = 255               # members of one group: a position fits d_best's byte
FUSE_STATS_WORDS = 4                 # uint64 words per member slot of uvad_fuse's d_stats: valid, speech, agree, best


class FuseCfg(C.Structure):      # uvad_fuse_cfg (12 bytes)
    _fields_ = [("mode", C.c_int), ("threshold", C.c_float), ("decide", C.c_float)]


class Cut(C.Structure):          # uvad_cut: one row of the cut table (32 bytes)
    _fields_ = [("row", C.c_int32), ("index", C.c_int32), ("first_frame", C.c_int32), ("n_frames", C.c_int32),
                ("first_sample", C.c_int64), ("n_samples", C.c_int64)]


class BinarizeCfg(C.Structure):  # uvad_binarize_cfg: thresholds and frame counts of uvad_binarize (24 bytes)
    _fields_ = [("onset", C.c_float), ("offset", C.c_float), ("min_on", C.c_int), ("min_off", C.c_int), ("pad_on", C.c_int),
                ("pad_off", C.c_int)]


GATE_FIRST, GATE_LAST, GATE_LOST, GATE_SHORT = 1, 2, 4, 8     # uvad_gate_seg.flags
GATE_UNSYNC = 16                                              # ... of uvad_gate_group_step: the group's members left lockstep


class GateSeg(C.Structure):      # uvad_gate_seg: one record of a gate step (32 bytes)
    _fields_ = [("index", C.c_int32), ("flags", C.c_int32), ("first_frame", C.c_int32), ("n_frames", C.c_int32), ("offset", C.c_int64),
                ("n", C.c_int32), ("n_stored", C.c_int32)]


class UvadError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"{ERR_NAMES.get(code, code)}: {msg}")
        self.code = code


# name -> (restype, argtypes); this table is also what tests check against include/uvad.h
SIGNATURES = {
    "uvad_abi_version": (C.c_int, []),
    "uvad_create": (C.c_int, [C.c_int, C.POINTER(FbankCfg), C.POINTER(ModelCfg), C.POINTER(C.c_void_p)]),
    "uvad_set_tables": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "uvad_set_weight": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.POINTER(C.c_int64), C.c_int]),
    "uvad_finalize": (C.c_int, [C.c_void_p]),
    "uvad_num_frames": (C.c_int64, [C.c_void_p, C.c_int64]),
    "uvad_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int, C.c_int64]),
    "uvad_fbank": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p]),
    "uvad_fbank_i16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p]),
    "uvad_classify": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                C.c_void_p, C.c_size_t, C.c_void_p]),
    "uvad_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p,
                               C.c_void_p, C.c_size_t, C.c_void_p]),
    "uvad_forward_i16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_size_t, C.c_void_p]),
    "uvad_sincnet_configure": (C.c_int, [C.c_void_p, C.POINTER(SincNetCfg)]),
    "uvad_sincnet_num_frames": (C.c_int64, [C.c_void_p, C.c_int64]),
    "uvad_sincnet_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int, C.c_int64]),
    "uvad_sincnet": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "uvad_forward_wav": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_size_t, C.c_void_p]),
    "uvad_sincnet_i16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "uvad_forward_wav_i16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_size_t, C.c_void_p]),
    "uvad_get_taps": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "uvad_stream_state_bytes": (C.c_size_t, [C.c_void_p, C.c_int]),
    "uvad_stream_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int, C.c_int]),
    "uvad_stream_reset": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "uvad_stream_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                   C.c_void_p, C.c_size_t, C.c_void_p]),
    "uvad_stream_peek": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int64), C.POINTER(C.c_int),
                                   C.POINTER(C.c_int)]),
    "uvad_stream_advance": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "uvad_window_state_bytes": (C.c_size_t, [C.c_void_p, C.c_int, C.c_int]),
    "uvad_window_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "uvad_window_reset": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "uvad_window_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                   C.c_void_p, C.c_size_t, C.c_void_p]),
    "uvad_window_peek": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int64)]),
    "uvad_window_advance": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "uvad_window_features": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_int), C.c_void_p]),
    "uvad_window_wav_state_bytes": (C.c_size_t, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "uvad_window_wav_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "uvad_window_wav_reset": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "uvad_window_wav_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                       C.c_void_p, C.c_size_t, C.c_void_p]),
    "uvad_window_wav_step_i16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                           C.c_void_p, C.c_size_t, C.c_void_p]),
    "uvad_window_wav_peek": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int64)]),
    "uvad_window_wav_advance": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "uvad_window_wav_features": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_int), C.c_void_p]),
    "uvad_window_slots_state_bytes": (C.c_size_t, [C.c_void_p, C.c_int, C.c_int]),
    "uvad_window_slots_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "uvad_window_slots_reset": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "uvad_window_slots_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "uvad_window_slots_features": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "uvad_window_wav_slots_state_bytes": (C.c_size_t, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "uvad_window_wav_slots_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "uvad_window_wav_slots_reset": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "uvad_window_wav_slots_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "uvad_window_wav_slots_step_i16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                                 C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "uvad_window_wav_slots_features": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "uvad_stream_slots_kmax": (C.c_int, [C.c_void_p, C.c_int]),
    "uvad_stream_slots_state_bytes": (C.c_size_t, [C.c_void_p, C.c_int]),
    "uvad_stream_slots_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int, C.c_int]),
    "uvad_stream_slots_reset": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "uvad_stream_slots_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "uvad_sliding_configure": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "uvad_sliding_count": (C.c_int64, [C.c_int64, C.c_int, C.c_int]),
    "uvad_sliding_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int, C.c_int64, C.c_int64, C.c_int]),
    "uvad_sliding_wav_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int, C.c_int64, C.c_int64, C.c_int]),
    "uvad_sliding_classify": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int,
                                        C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    **{name: (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_int,
                        C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p])
       for name in ("uvad_sliding_forward", "uvad_sliding_forward_i16", "uvad_sliding_forward_wav", "uvad_sliding_forward_wav_i16")},
    "uvad_ingest_configure": (C.c_int, [C.c_void_p, C.POINTER(IngestCfg)]),
    "uvad_ingest_set_taps": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "uvad_ingest_out_len": (C.c_int64, [C.c_void_p, C.c_int64]),
    "uvad_ingest_state_bytes": (C.c_size_t, [C.c_void_p, C.c_int]),
    "uvad_ingest": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p]),
    "uvad_ingest_lens": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "uvad_ingest_stream_reset": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]),
    "uvad_ingest_stream_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p,
                                          C.c_void_p]),
    "uvad_endpoint_state_bytes": (C.c_size_t, [C.c_void_p, C.c_int, C.POINTER(EndpointCfg)]),
    "uvad_endpoint_reset": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.POINTER(EndpointCfg), C.c_void_p]),
    "uvad_endpoint_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p,
                                     C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "uvad_intervals_to_labels": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                           C.c_void_p]),
    "uvad_score_configure": (C.c_int, [C.c_void_p, C.POINTER(ScoreCfg)]),
    "uvad_score_state_bytes": (C.c_size_t, [C.c_void_p]),
    "uvad_score_ws_bytes": (C.c_size_t, [C.c_void_p, C.c_int, C.c_int]),
    "uvad_score_reset": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "uvad_score_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t,
                                  C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "uvad_score_totals": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "uvad_head_train_configure": (C.c_int, [C.c_void_p, C.POINTER(HeadTrainCfg)]),
    "uvad_head_train_param_count": (C.c_int64, [C.c_void_p]),
    "uvad_head_train_state_bytes": (C.c_size_t, [C.c_void_p]),
    "uvad_head_train_ws_bytes": (C.c_size_t, [C.c_void_p, C.c_int, C.c_int]),
    "uvad_head_train_reset": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "uvad_head_train_grad": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                       C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                       C.c_void_p]),
    "uvad_head_train_apply": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "uvad_head_train_read": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p]),
    "uvad_head_train_commit": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "uvad_lstm_train_configure": (C.c_int, [C.c_void_p, C.POINTER(LstmTrainCfg)]),
    "uvad_lstm_train_param_count": (C.c_int64, [C.c_void_p]),
    "uvad_lstm_train_state_bytes": (C.c_size_t, [C.c_void_p]),
    "uvad_lstm_train_ws_bytes": (C.c_size_t, [C.c_void_p, C.c_int, C.c_int]),
    "uvad_lstm_train_reset": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "uvad_lstm_train_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                          C.c_size_t, C.c_void_p]),
    "uvad_lstm_train_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                           C.c_void_p, C.c_size_t, C.c_void_p]),
    "uvad_lstm_train_apply": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "uvad_lstm_train_read": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p]),
    "uvad_lstm_train_commit": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "uvad_lstm_train_set_dropout": (C.c_int, [C.c_void_p, C.c_float, C.c_uint64]),
    "uvad_dropout_apply": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_uint64, C.c_float, C.c_uint64, C.c_void_p]),
    "uvad_sincnet_train_configure": (C.c_int, [C.c_void_p, C.POINTER(SincNetTrainCfg)]),
    "uvad_sincnet_train_param_count": (C.c_int64, [C.c_void_p]),
    "uvad_sincnet_train_state_bytes": (C.c_size_t, [C.c_void_p]),
    "uvad_sincnet_train_ws_bytes": (C.c_size_t, [C.c_void_p, C.c_int, C.c_int64]),
    "uvad_sincnet_train_reset": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "uvad_sincnet_train_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                             C.c_void_p]),
    "uvad_sincnet_train_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                              C.c_void_p]),
    "uvad_sincnet_train_apply": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "uvad_sincnet_train_read": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p]),
    "uvad_sincnet_train_commit": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "uvad_optim_state_bytes": (C.c_size_t, [C.c_int]),
    "uvad_optim_ws_bytes": (C.c_size_t, [C.c_void_p]),
    "uvad_optim_reset": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(OptimCfg), C.POINTER(C.c_float), C.c_int, C.c_void_p]),
    "uvad_optim_set_lr_table": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_float), C.c_int, C.c_void_p]),
    "uvad_optim_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                  C.c_void_p, C.c_size_t, C.c_void_p]),
    "uvad_optim_read": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "uvad_optim_write": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "uvad_head_train_write": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p]),
    "uvad_lstm_train_write": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p]),
    "uvad_sincnet_train_write": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p]),
    "uvad_mix_state_bytes": (C.c_size_t, [C.POINTER(MixCfg), C.c_int]),
    "uvad_mix_ws_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "uvad_mix_reset": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(MixCfg), C.c_void_p, C.POINTER(C.c_int64), C.c_int, C.c_void_p]),
    "uvad_mix_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                C.c_void_p, C.c_size_t, C.c_void_p]),
    "uvad_mix_apply": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_uint64,
                                 C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]),
    "uvad_reverb_state_bytes": (C.c_size_t, [C.POINTER(ReverbCfg), C.c_int]),
    "uvad_reverb_ws_bytes": (C.c_size_t, [C.c_int]),
    "uvad_reverb_reset": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(ReverbCfg), C.c_void_p, C.POINTER(C.c_int64), C.c_int, C.c_void_p]),
    "uvad_reverb_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                   C.c_void_p, C.c_size_t, C.c_void_p]),
    "uvad_reverb_apply": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_uint64,
                                    C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]),
    "uvad_sampler_state_bytes": (C.c_size_t, [C.POINTER(SamplerCfg), C.c_int, C.c_int, C.c_int]),
    "uvad_sampler_ws_bytes": (C.c_size_t, [C.c_int]),
    "uvad_sampler_reset": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(SamplerCfg), C.c_void_p, C.c_int, C.POINTER(C.c_int64), C.c_int,
                                     C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_double), C.c_int,
                                     C.c_void_p]),
    "uvad_sampler_step": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]),
    "uvad_sampler_apply": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                     C.POINTER(C.c_int64), C.c_int64, C.c_uint64, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]),
    "uvad_sampler_read": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "uvad_sampler_write": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "uvad_cuts_max_per_row": (C.c_int, [C.POINTER(CutsCfg), C.c_int]),
    "uvad_cuts_max_samples": (C.c_int64, [C.POINTER(CutsCfg), C.c_int64]),
    "uvad_cuts_ws_bytes": (C.c_size_t, [C.c_void_p, C.c_int, C.c_int]),
    "uvad_cuts_table": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(CutsCfg),
                                  C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "uvad_cuts_gather": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                   C.c_int64, C.c_void_p, C.c_void_p]),
    "uvad_cuts_join_ws_bytes": (C.c_size_t, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "uvad_cuts_join": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                 C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "uvad_fuse_configure": (C.c_int, [C.c_void_p, C.POINTER(FuseCfg), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "uvad_fuse_ws_bytes": (C.c_size_t, [C.c_void_p, C.c_int, C.c_int]),
    "uvad_fuse": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                            C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "uvad_fuse_pick": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "uvad_binarize_ws_bytes": (C.c_size_t, [C.c_void_p, C.c_int, C.c_int]),
    "uvad_binarize": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.POINTER(BinarizeCfg), C.c_void_p, C.c_int,
                                C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "uvad_endpoint_hyst_lag": (C.c_int, [C.POINTER(BinarizeCfg)]),
    "uvad_endpoint_hyst_state_bytes": (C.c_size_t, [C.c_void_p, C.c_int, C.POINTER(BinarizeCfg)]),
    "uvad_endpoint_hyst_reset": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.POINTER(BinarizeCfg), C.c_void_p]),
    "uvad_endpoint_hyst_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p,
                                          C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "uvad_gate_state_bytes": (C.c_size_t, [C.c_void_p, C.c_int, C.POINTER(CutsCfg), C.c_int, C.c_int64]),
    "uvad_gate_history": (C.c_int64, [C.POINTER(CutsCfg), C.c_int, C.c_int]),
    "uvad_gate_max_out": (C.c_int64, [C.POINTER(CutsCfg), C.c_int, C.c_int, C.c_int64]),
    "uvad_gate_max_seg": (C.c_int, [C.POINTER(CutsCfg), C.c_int]),
    "uvad_gate_reset": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.POINTER(CutsCfg), C.c_int, C.c_int64, C.c_void_p]),
    "uvad_gate_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t,
                                 C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "uvad_gate_group_history": (C.c_int64, [C.POINTER(CutsCfg), C.c_int, C.c_int, C.c_int]),
    "uvad_gate_group_best_history": (C.c_int, [C.POINTER(CutsCfg), C.c_int, C.c_int, C.c_int]),
    "uvad_gate_group_max_out": (C.c_int64, [C.POINTER(CutsCfg), C.c_int, C.c_int, C.c_int]),
    "uvad_gate_group_state_bytes": (C.c_size_t, [C.c_void_p, C.POINTER(CutsCfg), C.c_int, C.c_int64, C.c_int]),
    "uvad_gate_group_reset": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(CutsCfg), C.c_int, C.c_int64, C.c_int, C.c_int, C.c_void_p]),
    "uvad_gate_group_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_void_p,
                                       C.c_void_p]),
    "uvad_classify_lens": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_size_t, C.c_void_p]),
    "uvad_forward_lens": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_size_t, C.c_void_p]),
    "uvad_forward_lens_i16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_size_t, C.c_void_p]),
    "uvad_fbank_lens": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "uvad_fbank_lens_i16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "uvad_sincnet_lens": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                    C.c_void_p]),
    "uvad_sincnet_lens_i16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                        C.c_void_p]),
    "uvad_forward_wav_lens": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_size_t, C.c_void_p]),
    "uvad_forward_wav_lens_i16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_size_t, C.c_void_p]),
    "uvad_median_filter_lens": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "uvad_label_runs_lens": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                       C.c_void_p]),
    "uvad_median_filter": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "uvad_label_runs": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "uvad_der_counts": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "uvad_set_gemm_mode": (C.c_int, [C.c_void_p, C.c_int]),
    "uvad_set_recurrent_tile": (C.c_int, [C.c_void_p, C.c_int]),
    "uvad_get_recurrent_tile": (C.c_int, [C.c_void_p]),
    "uvad_get_p2_on_fp8": (C.c_int, [C.c_void_p]),
    "uvad_get_sincnet_form": (C.c_int, [C.c_void_p]),
    "uvad_weights_shared_by": (C.c_int, [C.c_void_p]),
    "uvad_set_time_chunks": (C.c_int, [C.c_void_p, C.c_int]),
    "uvad_get_time_chunks": (C.c_int, [C.c_void_p]),
    "uvad_set_concurrent_steps": (C.c_int, [C.c_void_p, C.c_int]),
    "uvad_get_concurrent_steps": (C.c_int, [C.c_void_p]),
    "uvad_get_projection_grid": (C.c_int, [C.c_void_p]),
    "uvad_recurrent_tile_for": (C.c_int, [C.c_void_p, C.c_int]),
    "uvad_streams_overlap": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "uvad_set_timing": (C.c_int, [C.c_void_p, C.c_int]),
    "uvad_get_timing": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "uvad_get_layer_timing": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.c_int]),
    "uvad_last_error": (C.c_char_p, [C.c_void_p]),
    "uvad_destroy": (None, [C.c_void_p]),
}

_lib = None


def bind(lib):
    """Declare every prototype of SIGNATURES on `lib`.  The ABI number did not move when entries were appended (the ingest stage among
    them, the endpointer, the scoring stage, the speech cuts, the hysteresis decisions, the hysteresis endpointer, the speech gate, the cut-supervision join, the channel fusion and the group gate after it), so a library built from an older tree passes the version check: a symbol it lacks is a loud error here, by name."""
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            raise RuntimeError(f"libuvad.so does not export {name}: it was built from an older source tree; rebuild the library "
                               "(`make -C universal-voice-activity-detection_amd/csrc`)") from None
        fn.restype = res
        fn.argtypes = args
    return lib


def load():
    """dlopen libuvad.so and declare every prototype.  Raises (never falls back) if it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: the HIP extension has not been built. "
            "Run `python -c 'import __graft_entry__ as g; g.build()'` or "
            "`make -C universal-voice-activity-detection_amd/csrc`. There is no CPU fallback.")
    lib = bind(C.CDLL(LIB_PATH))
    got = lib.uvad_abi_version()
    if got != ABI_VERSION:
        raise RuntimeError(f"libuvad.so ABI {got} != binding ABI {ABI_VERSION}; rebuild the library")
    _lib = lib
    return lib


def check(lib, ctx, code):
    if code != UVAD_OK:
        msg = lib.uvad_last_error(ctx)
        raise UvadError(code, msg.decode() if msg else "")
