"""Host-side mirror of ``src.engines.vad_engine.VadModel`` (reference vad_engine.py:20-281),
inference and scoring surface: constructor arguments, ``.model`` / ``.model_name``, ``forward``,
``predict_step``, ``test_step``, ``validation_step``, ``_common_step`` and ``load_from_checkpoint``
keep their names, argument meaning and return shapes; what the reference logs through torchmetrics
is accumulated on the device (``uvad_score_*``) and read with ``test_metrics`` / ``validation_metrics``.
``adapt_head_step`` / ``adapt_head_commit`` fine-tune the head on the device (``uvad_head_train_*``); ``adapt_step`` /
``adapt_commit`` let the top LSTM layers learn with it (``uvad_lstm_train_*``); ``train_step`` / ``train_commit`` are the reference's
training step: every LSTM layer and the head learn, with nn.LSTM's dropout between the layers drawn on the device, and for a PyanNet the
SincNet front end learns from the raw waveform (``uvad_sincnet_train_*``).
``training_step`` and ``configure_optimizers`` themselves (Lightning's hooks; DDP) are outside the accelerated path and raise."""
import torch
import torch.nn as nn

from .models import PyanNet, PyanNet2
from .postprocess import median_filter, median_window, score_metrics


class VadModel(nn.Module):
    def __init__(self, model_name: str = "PyanNet2", model_dict: dict = None, learning_rate: float = 1e-3):
        super().__init__()
        model_dict = dict(model_dict or {})
        self.model_name = model_name
        self.model = PyanNet(**model_dict) if model_name == "PyanNet" else PyanNet2(**model_dict)
        self.model.build()
        self.learning_rate = learning_rate
        self._scorers = {}   # "test" / "val" -> (runtime, scoring state)

    # -- inference ---------------------------------------------------------------------------
    def forward(self, audio_feats: torch.Tensor) -> torch.Tensor:
        return self.model(audio_feats)

    def _common_step(self, batch, batch_idx, loss: bool = True):
        """vad_engine.py:247-278.  The reference also evaluates BCE against ``batch["is_voice"]``
        here (its value is unused by predict); it is computed only when labels are present.
        loss=False (test_step / validation_step) leaves the loss to the scoring stage, which sums it on the device:
        the NaN check below costs a synchronisation per batch."""
        x = batch["inputs"]
        y_pred = self.model(x.unsqueeze(1)) if self.model_name == "PyanNet" else self.model(x)
        y = batch.get("is_voice")
        want_loss, loss = loss, None
        if y is not None and want_loss:
            loss = nn.functional.binary_cross_entropy(y_pred.squeeze(-1), y.to(y_pred.device, y_pred.dtype))
            if torch.isnan(loss):
                return None
        return {"loss": loss}, y_pred, y

    def predict_step(self, batch, batch_idx=0, dataloader_idx=None):
        """vad_engine.py:204-211: probabilities -> threshold 0.5 -> median filter (49 taps at a
        10 ms hop, 25 at 20 ms) -> (batch, frames, 1) of 0/1."""
        _, y_pred, _ = self._common_step(batch, batch_idx)
        window = 0.02 if self.model.encoding_dim == 768 else 0.01
        labels = median_filter(y_pred.squeeze(-1), window=window)
        return labels.unsqueeze(-1)

    # -- checkpoints ---------------------------------------------------------------------------
    @classmethod
    def load_from_checkpoint(cls, checkpoint_path, map_location=None, **kwargs):
        """Accepts a Lightning ``.ckpt`` (dict with ``state_dict`` whose keys carry the ``model.``
        prefix) or a plain ``state_dict`` file.  Loaded with ``weights_only=True``.  As in the
        reference (predict.py:77) constructor arguments are NOT stored in the checkpoint, so
        ``model_dict`` must be passed for anything but the 768-dim default."""
        blob = torch.load(checkpoint_path, map_location=map_location or "cpu", weights_only=True)
        sd = blob.get("state_dict", blob) if isinstance(blob, dict) else blob
        obj = cls(**kwargs)
        own = {}
        for k, v in sd.items():
            if not torch.is_tensor(v):
                continue
            own[k if k.startswith("model.") else "model." + k] = v
        missing, unexpected = obj.load_state_dict(own, strict=False)
        missing = [m for m in missing if not m.endswith("num_batches_tracked")]
        if missing:
            raise RuntimeError(f"checkpoint is missing tensors: {missing[:4]}{'...' if len(missing) > 4 else ''}")
        return obj

    # -- scoring (vad_engine.py:128-202) ---------------------------------------------------------
    def _score_step(self, which, batch, batch_idx):
        _, y_pred, y = self._common_step(batch, batch_idx, loss=False)
        if y is None:
            raise ValueError(f'{which}_step needs batch["is_voice"]')
        probs = y_pred.squeeze(-1)
        rt = self.model.runtime(probs.device)
        held = self._scorers.get(which)
        if held is None or held[0] is not rt:
            window = 0.02 if self.model.encoding_dim == 768 else 0.01
            kernel = median_window(window) if which == "test" else 1    # test_step scores the median-filtered labels, validation_step the raw threshold
            held = self._scorers[which] = (rt, rt.score_open(points=[(0.5, kernel)]))
        gt = (y.to(probs.device) != 0).to(torch.uint8).reshape(probs.shape)
        rt.score_step(held[1], probs, gt, lengths=batch.get("lengths"))
        return rt.score_batch_loss(held[1])

    def test_step(self, batch, batch_idx=0):
        """vad_engine.py:167-202: the batch's probabilities against batch["is_voice"] at threshold 0.5 behind the reference's median window,
        accumulated on the device (one uvad_score_step, no copy to the host).  Returns the batch's mean loss as a 0-d tensor on the device
        without synchronising; where the reference's _common_step returns None for a NaN loss, the tensor is NaN.  batch["lengths"]
        (optional): valid frames per row."""
        return self._score_step("test", batch, batch_idx)

    def validation_step(self, batch, batch_idx=0):
        """vad_engine.py:128-165: as test_step without the median filter (kernel 1)."""
        return self._score_step("val", batch, batch_idx)

    def _metrics(self, which, reset):
        held = self._scorers.get(which)
        if held is None:
            raise RuntimeError(f"no {which}_step has run yet")
        rt, sc = held
        out = score_metrics(rt.score_read(sc), prefix=which)
        if reset:
            rt.score_reset(sc)
        return out

    def test_metrics(self, reset: bool = True) -> dict:
        """The reference's test_* names over every test_step since the last reset (postprocess.score_metrics: pooled, not Lightning's
        batch-weighted mean)."""
        return self._metrics("test", reset)

    def validation_metrics(self, reset: bool = True) -> dict:
        return self._metrics("val", reset)

    # -- head adaptation: the feed-forward layers and the classifier learn, the LSTM stack stays frozen (uvad_head_train_*) ----------
    def lstm_out(self, batch) -> torch.Tensor:
        """The frozen encoder's output (batch, frames, hidden x directions) for batch["inputs"]: what adapt_head_step trains on, and what
        a caller may cache across epochs as batch["lstm_out"]."""
        x = batch["inputs"]
        rt = self.model.runtime(x.device)
        if self.model_name == "PyanNet":
            x = rt.sincnet(x[:, 0, :] if x.dim() == 3 else x)
        rt.classify(x, want_logits=False, lengths=batch.get("lengths"))
        return rt.taps(lin=False)[0]

    def adapt_head_step(self, batch, batch_idx=0, accumulate: int = 1):
        """One micro-batch of head fine-tuning: batch["inputs"] through the frozen encoder (or batch["lstm_out"], cached taps, in its
        place), binary cross-entropy against batch["is_voice"] over the frames inside batch["lengths"] (optional), the gradients of
        linear.* and classifier.* accumulated on the device; every `accumulate` calls one Adam step (lr = self.learning_rate).
        Returns the batch's mean loss as a 0-d tensor on the device without synchronising, as test_step does."""
        y = batch.get("is_voice")
        if y is None:
            raise ValueError('adapt_head_step needs batch["is_voice"]')
        x = batch["lstm_out"] if batch.get("lstm_out") is not None else self.lstm_out(batch)
        rt = self.model.runtime(x.device)
        held = getattr(self, "_adapt", None)
        if held is None or held[0] is not rt:
            held = self._adapt = [rt, rt.head_train_open(lr=self.learning_rate), 0]
        gt = (y.to(x.device) != 0).to(torch.uint8).reshape(x.shape[:2])
        rt.head_train_grad(held[1], x, gt, lengths=batch.get("lengths"))
        held[2] += 1
        if held[2] % max(1, int(accumulate)) == 0:
            rt.head_train_apply(held[1])
        return rt.head_train_batch_loss(held[1])

    def adapt_head_commit(self):
        """Serve the adapted head from now on (uvad_head_train_commit) and write it into self.model's parameters, so that state_dict()
        and torch.save give the adapted checkpoint.  Synchronises."""
        held = getattr(self, "_adapt", None)
        if held is None:
            raise RuntimeError("no adapt_head_step has run yet")
        rt, h = held[0], held[1]
        rt.head_train_commit(h)
        params = dict(self.model.named_parameters())
        with torch.no_grad():
            for key, t in rt.head_train_state_dict(h).items():
                params[key].copy_(t.to(params[key].device))
        self.model._rt_stamp = self.model._stamp(rt.device)   # the runtime already holds these very tensors: no second upload

    # -- adaptation of the head AND the top LSTM layers (uvad_head_train_* + uvad_lstm_train_*) -------------------------------------
    def lstm_in(self, batch, lstm_layers: int = 1) -> torch.Tensor:
        """The frozen prefix's output for batch["inputs"]: the input of the lowest learning LSTM layer (the features themselves, or the
        SincNet output, when every layer learns).  What adapt_step trains on, and what a caller may cache as batch["lstm_in"]."""
        x = batch["inputs"]
        rt = self.model.runtime(x.device)
        if self.model_name == "PyanNet":
            x = rt.sincnet(x[:, 0, :] if x.dim() == 3 else x)
        return rt.lstm_train_input(x, lengths=batch.get("lengths"), layers=lstm_layers)

    _NO_SINCNET_LENGTHS = ("the SincNet front end normalises over whole rows (wav_norm1d and every instance norm), so per-row lengths are "
                           "not trained: batches of one length only")

    def _optim_of(self, rt, optim):
        """optim= of adapt_step / train_step -> an optimizer handle: the state VadRuntime.optim_open returned as it is, or one opened (once)
        from a dict of optim_open's options plus "lr_table" (default: the constant self.learning_rate)."""
        if "state" in optim:
            return optim
        held = getattr(self, "_optim", None)
        norm = {k: ([float(x) for x in v] if hasattr(v, "__len__") else v) for k, v in optim.items()}
        if held is None or held[0] is not rt or held[1] != norm:
            cfg = {k: v for k, v in optim.items() if k != "lr_table"}
            table = optim.get("lr_table")
            o = rt.optim_open(cfg, [self.learning_rate] if table is None else table)
            held = self._optim = [rt, norm, o]
            pending = getattr(self, "_pending_optimizer_state", None)
            if pending is not None and pending.get("optim") is not None:
                rt.optim_write(o, pending["optim"])
        return held[2]

    def _restore_pending(self, rt, hh, hl, hs=None):
        """load_optimizer_state's tensors into handles that were just opened."""
        st = getattr(self, "_pending_optimizer_state", None)
        if st is None:
            return
        for h, key, write in ((hh, "head", rt.head_train_write), (hl, "lstm", rt.lstm_train_write), (hs, "sincnet", rt.sincnet_train_write)):
            if h is not None and st.get(key) is not None:
                write(h, st[key])

    def optimizer_state(self) -> dict:
        """Everything a resumed run needs beside the weights, as CPU tensors: per family ("head", "lstm", "sincnet" when it learns) the
        masters, m, v and the scalar record (step, bias corrections, the LSTM's dropout draw ordinal), and "optim": the joint optimizer's
        record (applied and skipped steps) when adapt_step / train_step ran with optim=.  Synchronises."""
        held = getattr(self, "_adapt_full", None)
        if held is None:
            raise RuntimeError("no adapt_step has run yet")
        rt = held[0]
        pick = lambda r: {k: r[k] for k in ("weights", "m", "v", "scalars")}
        out = {"head": pick(rt.head_train_read(held[1])), "lstm": pick(rt.lstm_train_read(held[2]))}
        if len(held) > 4:
            out["sincnet"] = pick(rt.sincnet_train_read(held[4]))
        o = getattr(self, "_optim", None)
        if o is not None and o[0] is rt:
            out["optim"] = rt.optim_read(o[2])["record"]
        return out

    def load_optimizer_state(self, state: dict):
        """Restore what optimizer_state returned: into the training handles when adapt_step / train_step already opened them, otherwise
        into the handles the next such step opens (the handles take their shapes from that step's arguments)."""
        self._pending_optimizer_state = state
        held = getattr(self, "_adapt_full", None)
        if held is not None:
            self._restore_pending(held[0], held[1], held[2], held[4] if len(held) > 4 else None)
            o = getattr(self, "_optim", None)
            if o is not None and o[0] is held[0] and state.get("optim") is not None:
                held[0].optim_write(o[2], state["optim"])

    def _sincnet_step(self, batch, accumulate, sincnet_stages, dropout, seed, optim=None):
        """adapt_step with the top `sincnet_stages` SincNet stages learning: the waveform through sincnet_train_forward, every LSTM layer
        and the head above it, and the LSTM's input gradient back through the front end."""
        if batch.get("lengths") is not None:
            raise NotImplementedError(self._NO_SINCNET_LENGTHS)
        if self.model_name != "PyanNet":
            raise ValueError("sincnet_stages needs a PyanNet")
        stages = int(sincnet_stages)
        if not 1 <= stages <= 3:
            raise ValueError("sincnet_stages must lie in 0 .. 3")
        y = batch["is_voice"]
        wav = batch["inputs"]
        layers = self.model.hparams.lstm["num_layers"]       # the gradient reaches the front end only through every layer
        rt = self.model.runtime(wav.device)
        held = getattr(self, "_adapt_full", None)
        if held is None or held[0] is not rt or held[2]["layers"] != layers or len(held) < 5 or held[4]["first_stage"] != 3 - stages:
            held = self._adapt_full = [rt, rt.head_train_open(lr=self.learning_rate),
                                       rt.lstm_train_open(layers=layers, lr=self.learning_rate, dropout=dropout, seed=seed), 0,
                                       rt.sincnet_train_open(first_stage=3 - stages, lr=self.learning_rate)]
            self._restore_pending(rt, held[1], held[2], held[4])
        hh, hl, hs = held[1], held[2], held[4]
        hl["dropout"], hl["seed"] = dropout, int(seed) & 0xFFFFFFFFFFFFFFFF
        feats = rt.sincnet_train_forward(hs, wav)
        gt = (y.to(feats.device) != 0).to(torch.uint8).reshape(feats.shape[:2])
        out = rt.lstm_train_forward(hl, feats)
        _, gx = rt.head_train_grad(hh, out, gt, want_grad_x=True)
        gin = rt.lstm_train_backward(hl, feats, gx, want_grad_in=True)
        rt.sincnet_train_backward(hs, wav, gin)
        held[3] += 1
        if held[3] % max(1, int(accumulate)) == 0:
            if optim is not None:
                rt.optim_step(self._optim_of(rt, optim), head=hh, lstm=hl, sincnet=hs)
            else:
                rt.head_train_apply(hh)
                rt.lstm_train_apply(hl)
                rt.sincnet_train_apply(hs)
        return rt.head_train_batch_loss(hh)

    def adapt_step(self, batch, batch_idx=0, accumulate: int = 1, lstm_layers: int = 1, dropout=None, seed: int = 0, sincnet_stages: int = 0,
                   optim=None):
        """One micro-batch in which the head and the top `lstm_layers` LSTM layers learn: batch["lstm_in"] (the cached frozen prefix) or
        batch["inputs"] through it, the learning layers' forward pass with kept activations, the head's loss and backward pass as
        adapt_head_step's, backpropagation through time from its input gradient; every `accumulate` calls one Adam step on both
        states (lr = self.learning_rate).  dropout: nn.LSTM's dropout between the learning layers, a fresh mask per call (None: none,
        the frozen prefix never has any); seed: the masks' seed.  sincnet_stages = k > 0 (PyanNet): the top k stages of the SincNet front
        end learn too, from the waveform batch["inputs"] (B, 1, S) or (B, S) -- every LSTM layer then learns, whatever lstm_layers says,
        and batch["lengths"] must be None.  optim: None -- every state takes its own plain Adam step (the _apply calls); a dict of
        VadRuntime.optim_open's options (plus "lr_table"), or the state optim_open returned -- the step ends in ONE uvad_optim_step over
        all learning states instead: the global gradient norm and its clipping, weight decay, the table's learning rate, a non-finite
        step skipped.  Returns the batch's mean loss as a 0-d tensor on the device without synchronising."""
        y = batch.get("is_voice")
        if y is None:
            raise ValueError('adapt_step needs batch["is_voice"]')
        dropout = 0.0 if dropout is None else float(dropout)
        if not 0.0 <= dropout < 1.0:
            raise ValueError("dropout must lie in [0, 1)")
        if int(sincnet_stages) != 0:
            return self._sincnet_step(batch, accumulate, sincnet_stages, dropout, seed, optim)
        x = batch["lstm_in"] if batch.get("lstm_in") is not None else self.lstm_in(batch, lstm_layers)
        rt = self.model.runtime(x.device)
        held = getattr(self, "_adapt_full", None)
        if held is None or held[0] is not rt or held[2]["layers"] != int(lstm_layers) or len(held) > 4:   # (a SincNet handle of an earlier
            held = self._adapt_full = [rt, rt.head_train_open(lr=self.learning_rate),                      # sincnet_stages > 0 step: start anew)
                                       rt.lstm_train_open(layers=lstm_layers, lr=self.learning_rate, dropout=dropout, seed=seed), 0]
            self._restore_pending(rt, held[1], held[2])
        hh, hl = held[1], held[2]
        hl["dropout"], hl["seed"] = dropout, int(seed) & 0xFFFFFFFFFFFFFFFF      # the handle re-asserts them before every call
        lengths = batch.get("lengths")
        gt = (y.to(x.device) != 0).to(torch.uint8).reshape(x.shape[:2])
        out = rt.lstm_train_forward(hl, x, lengths=lengths)
        _, gx = rt.head_train_grad(hh, out, gt, lengths=lengths, want_grad_x=True)
        rt.lstm_train_backward(hl, x, gx, lengths=lengths)
        held[3] += 1
        if held[3] % max(1, int(accumulate)) == 0:
            if optim is not None:
                rt.optim_step(self._optim_of(rt, optim), head=hh, lstm=hl)
            else:
                rt.head_train_apply(hh)
                rt.lstm_train_apply(hl)
        return rt.head_train_batch_loss(hh)

    def adapt_commit(self):
        """Serve the adapted head and LSTM layers from now on (uvad_lstm_train_commit + uvad_head_train_commit) and write them into
        self.model's parameters, so that state_dict() and torch.save give the adapted checkpoint.  Synchronises."""
        held = getattr(self, "_adapt_full", None)
        if held is None:
            raise RuntimeError("no adapt_step has run yet")
        rt, hh, hl = held[0], held[1], held[2]
        hs = held[4] if len(held) > 4 else None
        front = {}
        if hs is not None:                                   # the front end first: each commit re-finalizes with what is set so far
            rt.sincnet_train_commit(hs)
            front = rt.sincnet_train_state_dict(hs)          # low_hz_ and band_hz_ among them
        rt.lstm_train_commit(hl)
        rt.head_train_commit(hh)
        params = dict(self.model.named_parameters())
        with torch.no_grad():
            for key, t in list(rt.head_train_state_dict(hh).items()) + list(rt.lstm_train_state_dict(hl).items()) + list(front.items()):
                if key not in params:   # the ModuleList-of-LSTMs variant: lstm.{k}.weight_ih_l0[_reverse]
                    name, k = key[len("lstm."):].split("_l", 1)
                    key = f"lstm.{k.replace('_reverse', '')}.{name}_l0" + ("_reverse" if k.endswith("_reverse") else "")
                params[key].copy_(t.to(params[key].device))
        self.model._rt_stamp = self.model._stamp(rt.device)   # the runtime already holds these very tensors: no second upload

    # -- training from initialisation: every LSTM layer and the head learn (PyanNet2) -----------------------------------------------
    def train_step(self, batch, batch_idx=0, accumulate: int = 1, optim=None):
        """The reference's training_step on the device: adapt_step with every LSTM layer learning, the model's configured dropout between
        the layers (self.model.train_dropout) and the masks seeded from torch.initial_seed().  A PyanNet takes the waveform batch
        (B, 1, S) or (B, S) and its whole SincNet front end learns with the rest; its batch must not carry lengths.  optim: adapt_step's."""
        if self.model_name == "PyanNet" and batch.get("lengths") is not None:    # before the model or the device is touched
            raise NotImplementedError("train_step: " + self._NO_SINCNET_LENGTHS)
        return self.adapt_step(batch, batch_idx, accumulate=accumulate, lstm_layers=self.model.hparams.lstm["num_layers"],
                               dropout=self.model.train_dropout, seed=torch.initial_seed(),
                               sincnet_stages=3 if self.model_name == "PyanNet" else 0, optim=optim)

    def train_commit(self):
        """adapt_commit: serve the trained tensors and write them into self.model's parameters."""
        self.adapt_commit()

    # -- Lightning's own hooks stay outside the accelerated path -----------------------------------
    def training_step(self, *a, **k):
        raise NotImplementedError("training is outside the accelerated inference path (SURVEY.md section 2, rows 6/12)")

    configure_optimizers = training_step
