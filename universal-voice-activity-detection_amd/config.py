"""``load_config()`` with the reference's key names (config/config.py:4-438) for the inference
path.  The reference returns an ``ml_collections.ConfigDict`` (not installed here); ``ConfigDict``
below gives the same attribute + mapping access, including ``**config`` splatting (main.py:34-44).
Corpus / training / W&B keys of the reference are out of scope and omitted; a manifest-free
``input`` block (synthetic signal or wav files) replaces the lhotse manifests on cluster paths."""
import os


class ConfigDict(dict):
    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k) from None

    def __setattr__(self, k, v):
        self[k] = v


def load_config() -> ConfigDict:
    cfg = ConfigDict()

    cfg.task = "run"            # only "run" is in scope (reference: wer/download/prepare/... are data plumbing)
    cfg.function = "predict"    # "predict" | "test" (scoring against label files: input.labels) | "adapt" (head fine-tuning on them) |
                                # "train" (scripts.train_vad: every LSTM layer and the head learn from torch's initialisation)

    cfg.seed = 42
    cfg.device = "gpu"          # the HIP path needs a GPU; "cpu" raises (no fallback)
    cfg.num_devices = 1
    cfg.distributed_training = False

    cfg.feature_extractor = os.environ.get("UVAD_FEATURE_EXTRACTOR", "fbank")   # "fbank" (log-mel + PyanNet2) | "sincnet" (PyanNet);
                                                                                # wav2vec2 / hubert are out of scope
    cfg.frame_shift = 0.01 if cfg.feature_extractor == "fbank" else 0.02

    cfg.supported_models = ["PyanNet", "PyanNet2"]
    cfg.model_name = "PyanNet" if cfg.feature_extractor == "sincnet" else "PyanNet2"

    cfg.model_dict = ConfigDict()
    if cfg.feature_extractor == "sincnet":
        cfg.model_dict.encoding_dim = 60
    elif cfg.feature_extractor == "fbank":
        cfg.model_dict.encoding_dim = 80
    else:
        cfg.model_dict.encoding_dim = 768

    cfg.max_duration = 400      # seconds of audio per batch, as the reference's sampler
    # cut geometry of the reference's recipes (src/datasets/ami/utils.py:107,163): 5 s windows, tails of <= 3 s dropped, features
    # padded to the window; window_seconds = None runs whole recordings in one pass instead (not what the reference does)
    # function == "train" cuts its cached features into rows of window_seconds too, every tail kept as a shorter row with its length
    cfg.window_seconds = 5.0
    cfg.min_window_seconds = 3.0
    # with window_seconds = None: recordings of different lengths share a batch (sorted by length, padded size within max_duration),
    # each row classified on its own length (uvad_forward_lens); False runs recordings of equal length together only
    cfg.ragged_batches = False
    # hop_seconds = None: the cuts above.  A number: overlapping windows of window_seconds every hop_seconds over whole recordings, each
    # run from zero state, a frame's probability the weighted mean over the windows that cover it (uvad_sliding_forward); no tail is
    # dropped and features are slices of each recording's continuous feature stream
    cfg.hop_seconds = None
    cfg.sliding_weights = "hamming"   # "rect" | "hamming" (postprocess.sliding_weights)
    cfg.sliding_group = 512           # windows per classifier launch: bounds the workspace, not the result
    # cuts = None: nothing more.  A dict {"buffer": s, "split": bool, "window": 10.0, "min": 0.1, "write_dir": None} (the options of the
    # reference's get_new_cuts, seconds): every result gains "cuts", [(start_s, end_s, first_sample, n_samples)] -- the runs widened by
    # buffer and merged, with split cut to at most window seconds, remainders of min seconds or less dropped (uvad_cuts_table); with
    # write_dir one 16 kHz wav per cut is written there (uvad_cuts_gather)
    cfg.cuts = None
    # supervisions / alignments = None: nothing more.  With cuts, {recording_id: path or [(start_s, end_s, text)]} (a file of
    # `start<TAB>end<TAB>text` lines, postprocess.read_supervisions): every cut gains the indices of the recording's supervisions that
    # overlap it and their concatenated text, every result the reference's seven counters (uvad_cuts_join).  alignments has one entry
    # per word; a word belongs to the cut that holds it whole, and with both given the words supply the text
    cfg.supervisions = None
    cfg.alignments = None
    # binarize = None: labels are threshold 0.5 + median, as the reference's predict_step.  A dict in seconds {"onset": 0.5, "offset": None,
    # "min_duration_on": 0.0, "min_duration_off": 0.0, "pad_onset": 0.0, "pad_offset": 0.0}: hysteresis decisions instead (uvad_binarize)
    # -- speech turns on at onset and off below offset, runs are padded, pauses shorter than min_duration_off filled and intervals shorter
    # than min_duration_on dropped; with cuts, pass buffer = 0 there if padding was applied here
    cfg.binarize = None
    # fuse = None: with input.channels = "all" every channel of a file is a recording of its own (rec-ch0, rec-ch1, ...).  A dict {"mode":
    # "max" | "mean" | "vote", "threshold": 0.5, "decide": None}: the channels' probabilities are fused on the device (uvad_fuse) and each
    # file gives ONE result, with "channel_stats"; with cuts each cut's audio comes from the channel that heard it best and carries
    # "channel" (uvad_fuse_pick).  function = "test" then scores the fused row of a multi-channel file against its label file
    cfg.fuse = None

    cfg.experiments_dir = os.environ.get("UVAD_EXPERIMENTS_DIR", "experiments")
    cfg.load_checkpoint = False
    cfg.checkpoint_path = ""
    cfg.weights_seed = 1234     # used when load_checkpoint is False (no checkpoint ships with the reference)
    cfg.weights_scale = 4.0

    # function == "adapt" (scripts.adapt_vad): the feed-forward layers and the classifier learn, the LSTM stack stays frozen
    cfg.learning_rate = 1e-3
    cfg.max_epochs = 10
    cfg.check_val_every_n_epoch = 1
    cfg.accumulate_grad_batches = 1
    cfg.adapted_checkpoint_path = ""    # "" = experiments_dir/adapted.ckpt
    cfg.adapt_lstm_layers = 0           # top LSTM layers that learn with the head (VadModel.adapt_step); 0 = the head alone, as before

    # function == "train": noise augmentation of the training phase, drawn anew for every batch on the device (uvad_mix_step; validation is
    # never mixed).  noise = {"paths": [wav files], "snr": (10, 20), "mix_prob": 0.5} or None.  The reference's keys give the same:
    # enable_musan (its default) with musan.paths, the noise recordings -- an empty list (no corpus ships) trains on clean audio
    cfg.noise = None
    cfg.enable_musan = True
    cfg.musan = ConfigDict()
    cfg.musan.paths = []
    cfg.musan.snr = (10, 20)
    cfg.musan.mix_prob = 0.5
    # ... and reverberation, in front of the noise (uvad_reverb_step): reverb = {"paths": [wav files, one room impulse response each],
    # "prob": 0.5, "normalize": True, "align": True, "max_seconds": None} or None
    cfg.reverb = None

    # function == "train" / "adapt" with adapt_lstm_layers: the joint optimizer step (uvad_optim_step).  All at their defaults: every state
    # takes its own plain Adam step, as before.  gradient_clip_val: the global gradient norm is clipped to it (0 = off); weight_decay with
    # adamw (False: L2 into the gradient, torch.optim.Adam(weight_decay=); True: AdamW); lr_schedule: None or {"name": "constant" | "warmup" |
    # "linear" | "cosine" | "step", ...} (scripts.lr_schedule_table); skip_nonfinite: a step whose gradient norm is not finite is skipped.
    # stop_after_epoch: end the run after that epoch with its checkpoint (0 = run to max_epochs); the same configuration with
    # load_checkpoint then continues it.
    cfg.gradient_clip_val = 0.0
    cfg.weight_decay = 0.0
    cfg.adamw = False
    cfg.lr_schedule = None
    cfg.skip_nonfinite = False
    cfg.stop_after_epoch = 0

    cfg.predict_output_dir = os.environ.get("UVAD_PREDICT_DIR", "")   # "" = do not write files
    cfg.window_type = "povey"   # lhotse default; BASELINE cfg 2 uses "hamming"

    # manifest-free input (BASELINE cfg 1: one 30 s 16 kHz utterance)
    cfg.input = ConfigDict()
    cfg.input.kind = "synthetic"      # "synthetic" | "wav"
    cfg.input.paths = []              # wav files when kind == "wav": 16 kHz 16-bit as they are; other rates, G.711 (A-law / mu-law) and
                                      # multi-channel files through the ingest stage (decode, channels to rows, resampling to 16 kHz)
    cfg.input.labels = []             # function == "test": one label file per path, `start<TAB>end<TAB>LABEL` lines (get_audacity_labels)
    cfg.input.val_paths = []          # function == "adapt": held-out wav files and their label files (empty: the training files)
    cfg.input.val_labels = []
    cfg.input.channels = "first"      # "first": channel 0 only (the reference's to_mono(mono_downmix=False)[0]); "all": every channel a
                                      # recording of its own, "-ch<N>" appended to its id
    cfg.input.num_utterances = 1
    cfg.input.seconds = 30.0
    cfg.input.seed = 1000
    return cfg
