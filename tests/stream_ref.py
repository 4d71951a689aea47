"""Plain restatement of the framing arithmetic of a causal stream (uvad_stream_step), from the definition only.

Centred framing (snip_edges = 0): frame t spans the samples [t * sh - n_left, t * sh - n_left + L) with n_left = (L - sh) / 2 (the
samples left of 0 are the mirror of the first ones, so they arrive with the first chunk).  Frame t is complete once the feed holds
n >= t * sh - n_left + L samples.  Everything below is a loop over frames: no closed form, nothing of the library's stream_plan()."""


def frames_complete(n, L=400, sh=160):
    """Number of frames whose last sample lies inside the first n samples of a feed."""
    n_left = (L - sh) // 2
    t = 0
    while t * sh - n_left + L <= n:
        t += 1
    return t


def k_schedule(chunk, steps, L=400, sh=160):
    """The number of frames each of `steps` steps of `chunk` samples completes."""
    out, done = [], 0
    for i in range(1, steps + 1):
        now = frames_complete(i * chunk, L, sh)
        out.append(now - done)
        done = now
    return out


def frames_covering(sample, n_frames, L=400, sh=160):
    """The frames t < n_frames whose span holds the sample (ascending; the mirrored left edge counts: sample s < n_left is also
    read at position -1 - s)."""
    n_left = (L - sh) // 2
    hit = []
    for t in range(n_frames):
        lo, hi = t * sh - n_left, t * sh - n_left + L
        if lo <= sample < hi or (sample < n_left and lo <= -1 - sample < hi):
            hit.append(t)
    return hit


def step_and_position(ks, t):
    """(step, position inside that step's new frames) of frame t under the schedule ks."""
    done = 0
    for i, k in enumerate(ks):
        if t < done + k:
            return i, t - done
        done += k
    raise ValueError(f"frame {t} is not emitted by {len(ks)} steps")
