"""uvad_set_concurrent_steps: the persistent projection (and head) grids of a context whose caller keeps n steps in flight leave the other
steps' recurrences their CUs (include/uvad.h).  The grid getter must report what the rule gives -- that is what keeps the bit
comparisons from passing vacuously -- and no output bit may move: the tile queue hands every tile out once whatever the grid."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
F = 64
STEPS = (1, 2, 3, 5, 12)
MAX_RESERVE_SHARE = 0.5   # above this share of the chip in reserve the grids are whole again (profiles/slot_grid.json)


def rule(n_cu, n, rec_cus, per):
    """Workgroups of a weight-stationary projection launch (include/uvad.h, uvad_set_concurrent_steps)."""
    reserve = (n - 1) * rec_cus
    if n == 1 or reserve > MAX_RESERVE_SHARE * n_cu:
        return max(per, n_cu // per * per)
    return max(per, (n_cu - reserve) // per * per)


def make(hidden, layers=2):
    import uvad_amd
    from uvad_amd.synth import seed_weights
    m = uvad_amd.PyanNet2(lstm={"hidden_size": hidden, "num_layers": layers, "bidirectional": True}, encoding_dim=F)
    m.build()
    seed_weights(m, 1234, 2.0)
    m = m.to(DEV).eval()
    return m, m.runtime(DEV)


def feats(B, T):
    g = torch.Generator().manual_seed(7)
    return (torch.randn(B, T, F, generator=g) * 2.0).to(DEV)


# (hidden, B, T, tile): 16 384 rows each, the smallest round shapes the weight-stationary kernel takes on 256 CUs
@pytest.mark.parametrize("hidden,B,T,tile", [(128, 256, 64, 16), (128, 256, 64, 4), (64, 64, 256, 4)])
def test_rule_takes_effect_and_bits_do_not_move(hidden, B, T, tile):
    m, rt = make(hidden)
    n_cu = torch.cuda.get_device_properties(DEV).multi_processor_count
    per = 8 * (4 * hidden * 2 // 128)
    tiles = (B + 3) // 4
    rec_cus = ((tiles + 3) // 4 if tile == 16 else tiles) * 2
    rt.set_recurrent_tile(tile)
    rt.set_time_chunks(1)
    x = feats(B, T)
    want = None
    for n in STEPS:
        rt.set_concurrent_steps(n)
        assert rt.concurrent_steps() == n
        logits, probs = rt.classify(x)
        torch.cuda.synchronize(DEV)
        assert rt.recurrent_tile() == tile and rt.time_chunks() == 1
        grid = rt.projection_grid()
        print(f"hidden {hidden} tile {tile} n {n}: projection grid {grid} (rule {rule(n_cu, n, rec_cus, per)}, {n_cu} CUs, rec_cus {rec_cus})")
        assert grid == rule(n_cu, n, rec_cus, per)
        if n == 1:
            want = (logits.clone(), probs.clone())
        else:
            assert torch.equal(logits, want[0]) and torch.equal(probs, want[1])
    rt.set_concurrent_steps(1)


def test_small_launches_run_the_same_kernels():
    m, rt = make(128)
    x = feats(8, 100)
    rt.set_time_chunks(1)
    want = None
    for n in STEPS:
        rt.set_concurrent_steps(n)
        logits, _ = rt.classify(x)
        torch.cuda.synchronize(DEV)
        assert rt.projection_grid() == 0          # below the weight-stationary threshold: the tile-streaming projection, whatever n
        if want is None:
            want = logits.clone()
        assert torch.equal(logits, want)


def test_in_flight_steps_equal_a_single_call():
    import uvad_amd
    from uvad_amd.synth import seed_weights, synth_pcm_device
    m = uvad_amd.PyanNet2(encoding_dim=F)
    m.build()
    seed_weights(m, 1234, 2.0)
    m.attach_fbank(uvad_amd.FbankConfig(num_filters=F, window_type="hamming"))
    m = m.to(DEV).eval()
    B, T = 64, 300
    S = T * 160
    n_cu = torch.cuda.get_device_properties(DEV).multi_processor_count
    pipe = uvad_amd.ForwardPipeline(m, DEV, depth=3, recurrent_tile=16)
    try:
        assert pipe.runtimes[0].num_frames(S) == T
        assert all(r.concurrent_steps() == 3 for r in pipe.runtimes)
        pcm = synth_pcm_device(B, S, seed=11, device=DEV)
        alone = pipe.runtimes[0].forward(pcm, want_probs=False)[0].clone()
        torch.cuda.synchronize(DEV)
        rec_cus = ((B // 4 + 3) // 4) * 2
        assert pipe.runtimes[0].projection_grid() == rule(n_cu, 3, rec_cus, 64)
        pending = [pipe.submit(pcm) for _ in range(12)]
        for p in pending:
            assert torch.equal(p.result()[0], alone)
        pipe.synchronize()
        pipe.set_active_depth(2)
        pipe.submit(pcm).wait()
        assert pipe.runtimes[0].concurrent_steps() == 2
        assert pipe.runtimes[0].projection_grid() == rule(n_cu, 2, rec_cus, 64)
    finally:
        pipe.close()


def test_arguments():
    from uvad_amd._lib import UvadError
    m, rt = make(128, layers=1)
    assert rt.concurrent_steps() == 1
    for bad in (0, -3):
        with pytest.raises(UvadError) as e:
            rt.set_concurrent_steps(bad)
        assert e.value.code == -1
    assert rt.concurrent_steps() == 1
