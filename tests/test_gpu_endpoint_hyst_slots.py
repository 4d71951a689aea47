"""GPU tests (-m gpu) of the hysteresis endpointer behind both slot pools (window_slots_open / wav_window_slots_open with endpoint={"onset":
.., "offset": .., "min_on": .., ..}), at the pool shapes of tests/test_gpu_endpoint_slots.py, whose models, input and session schedule
are used as they are: the hysteresis step is enqueued right behind the pool step -- inside the one captured graph under graphs=True -- on
the pool's probabilities, counts and flags.  Its events, counts, active byte and labels equal the frame-loop simulator
(tests/endpoint_hyst_ref.py) applied to the probabilities the same run emitted, the pool's own outputs are byte-identical to a pool opened
without an endpointer, and mixed or unknown parameter sets are refused."""
import numpy as np
import pytest
import torch

import binarize_ref as br
import endpoint_hyst_ref as hr
import endpoint_ref as er
import test_gpu_endpoint_slots as es

pytestmark = pytest.mark.gpu

STEPS = es.STEPS
_INTS = {"min_on": 3, "min_off": 2, "pad_on": 1, "pad_off": 2}


def _check(open_pool, step, x, flags, chunk, B):
    """onset and offset: the 45th and 25th percentile of the probabilities the pool emits for this input (taken from the run without an
    endpointer), so that a model whose outputs sit on one side of 0.5 still gives frames of all three classes."""
    plain, st0 = es._run(open_pool, step, x, flags, chunk, None, False)
    assert "endpoint" not in st0 and "probs" not in st0
    emitted = np.concatenate([rec["logits"][b, :int(rec["counts"][b])] for rec in plain for b in range(B)]).astype(np.float64)
    assert len(emitted) > 20
    sig = lambda z: float(np.float32(1.0 / (1.0 + np.exp(-z))))
    EP = dict(_INTS, onset=sig(np.percentile(emitted, 45)), offset=sig(np.percentile(emitted, 25)))
    assert EP["offset"] < EP["onset"]
    q = br.cfg(**EP)
    for graphs in (False, True):
        got, st = es._run(open_pool, step, x, flags, chunk, EP, graphs)
        if graphs:
            assert st["graphs"] == 1                                        # pool step and endpoint step in the one capture
        ld, ep = st["out"].shape[1], st["endpoint"]
        assert ep["ld_in"] == ld and ep["max_events"] == ld + 1 and ep["lag"] == hr.lag(q) == 7 and ep["labels"].shape[1] == ld + 7
        # the pool's own outputs do not move
        for s in range(STEPS):
            assert np.array_equal(got[s]["counts"], plain[s]["counts"]), (graphs, s)
            for b in range(B):
                n = int(plain[s]["counts"][b])
                assert got[s]["logits"][b, :n].tobytes() == plain[s]["logits"][b, :n].tobytes(), (graphs, s, b)
        # the endpointer on the probabilities this very run emitted
        counts = np.stack([g["counts"] for g in got])
        probs = np.stack([g["probs"] for g in got])
        want = hr.simulate(probs, counts, flags, q)
        n_events, actives = 0, set()
        for s, row in enumerate(want):
            for b, (y, ev, active) in enumerate(row):
                assert got[s]["ev_counts"][b] == len(ev), (graphs, s, b, ev)
                assert got[s]["events"][b, :len(ev)].tolist() == [list(e) for e in ev], (graphs, s, b)
                assert got[s]["active"][b] == active and got[s]["lab_counts"][b] == len(y), (graphs, s, b)
                assert np.array_equal(got[s]["labels"][b, :len(y)], y), (graphs, s, b)
                n_events += len(ev)
                actives.add(active)
        # ended sessions: the whole-row answer
        for b, s0, s1, ended in er.sessions(counts, flags):
            if ended and flags[s0, b] & 1:
                row = er.session_row(probs, counts, b, s0, s1)
                evs = [tuple(e) for s in range(s0, s1 + 1) for e in got[s]["events"][b, :got[s]["ev_counts"][b]].tolist()]
                labs = np.concatenate([got[s]["labels"][b, :got[s]["lab_counts"][b]] for s in range(s0, s1 + 1)])
                y, iv = hr.whole(row, q)
                assert evs == hr.events_of(iv) and labs.tobytes() == y.tobytes(), (graphs, b, s0)
        print(f"graphs={graphs}: onset {q.onset:.6f}, offset {q.offset:.6f}, {n_events} events, active bytes {sorted(actives)} over {int(counts.sum())} frames")
        assert n_events > 0 and actives >= {0, 1}


def _refusals(open_pool):
    from uvad_amd.postprocess import binarize_config
    for bad in ({"onset": 0.6, "kernel": 5}, {"pad": 2, "pad_on": 2}, {"threshold": 0.5, "offset": 0.4},      # mixed sets
                {"onset": 0.6, "taps": 5}, {"taps": 5}, {"min_duration_on": 0.1},                              # unknown keys
                {"kernel": 4}, {"onset": 0.3, "offset": 0.6}, {"min_on": -1}):                                  # bad values
        with pytest.raises(ValueError):
            open_pool(endpoint=bad)
    with pytest.raises(ValueError, match=r"unknown endpoint parameters \['taps'\] \(kernel, pad, threshold\)$"):
        open_pool(endpoint={"taps": 5})
    st = open_pool(endpoint=binarize_config(0.6, 0.4, 0.05, 0.03, 0.01, 0.02))                                 # seconds -> the dict, passed as it is
    assert (st["endpoint"]["min_on"], st["endpoint"]["min_off"], st["endpoint"]["pad_on"], st["endpoint"]["pad_off"]) == (5, 3, 1, 2)
    assert st["endpoint"]["lag"] == 5 + 1 + 2 + 2


def test_logmel_pool_with_hysteresis_endpoint():
    B, chunk, W, L = 3, 320, 50, 7
    m, rt = es._logmel_model()
    open_pool = lambda **kw: rt.window_slots_open(B, chunk, window=W, lookahead=L, **kw)
    _check(open_pool, rt.window_slots_step, es._pcm(B, chunk, 21), es._flags(B), chunk, B)
    _refusals(open_pool)


def test_waveform_pool_with_hysteresis_endpoint():
    B, chunk, W, L = 2, 320, 60, 7
    m, rt = es._wav_model()
    open_pool = lambda **kw: rt.wav_window_slots_open(B, chunk, window=W, lookahead=L, **kw)
    _check(open_pool, rt.wav_window_slots_step, es._pcm(B, chunk, 22), es._flags(B), chunk, B)
    _refusals(open_pool)
