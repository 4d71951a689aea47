"""CPU restatement of the joint optimizer step (uvad_optim_step, include/uvad.h) in numpy, in two modes: f32, operation by operation in the
documented order (what the device must reproduce bit for bit), and float64 (what torch's clip_grad_norm_ + Adam / AdamW compute).  A
family is a dict {"w", "m", "v", "t", "bc1", "bc2"} (head_train_ref.adam_init's moments plus the masters); a step takes, per family, None (absent)
or (family, accumulated gradient, frames) and returns the new families, the new optimizer counts and the record uvad_optim_read gives."""
import numpy as np

F32 = np.float32
CHUNK, LANES = 4096, 256


def family(w, f64=False):
    dt = np.float64 if f64 else F32
    w = np.array(w, dt).reshape(-1)
    return {"w": w, "m": np.zeros_like(w), "v": np.zeros_like(w), "t": 0, "bc1": dt(0.0), "bc2": dt(0.0)}


def default_cfg(**kw):
    cfg = {"beta1": 0.9, "beta2": 0.999, "eps": 1e-8, "max_norm": 0.0, "weight_decay": 0.0, "decoupled": False, "skip_nonfinite": False,
           "lr_scale": (1.0, 1.0, 1.0)}
    cfg.update(kw)
    return cfg


def chunk_partials(g):
    """The sums of squares of an f32 gradient per chunk of 4096 parameters, in the device's order: lane l of 256 adds the exact double
    squares of elements l, l + 256, ..., l + 3840 of its chunk in that order from +0; then lane l += lane l + o for o = 128, 64, ..., 1."""
    g = np.asarray(g, F32).reshape(-1)
    out = []
    for j0 in range(0, g.size, CHUNK):
        c = np.zeros(CHUNK, np.float64)
        part = g[j0:j0 + CHUNK].astype(np.float64)
        c[:part.size] = part * part                  # exact: 24-bit x 24-bit significands
        lanes = np.zeros(LANES, np.float64)
        for row in c.reshape(CHUNK // LANES, LANES):
            lanes = lanes + row                      # a lane past the ragged tail adds +0, which changes nothing
        o = LANES // 2
        while o >= 1:
            lanes[:o] = lanes[:o] + lanes[o:2 * o]
            o //= 2
        out.append(lanes[0])
    return out


def sum_squares(grads):
    """S over the participating families' f32 gradients in the order given (head, LSTM, SincNet): chunk sums added in chunk order."""
    S = np.float64(0.0)
    for g in grads:
        for p in chunk_partials(g):
            S = S + p
    return S


def _one_minus(b):
    """1 - beta as the library forms it: in f64 from the shortest decimal that rounds to the f32, rounded to f32 once."""
    return F32(1.0 - float(str(F32(b))))


def step(fams, opt, cfg, table, f64=False):
    """fams: three entries, None or (family, acc, frames); opt: {"t", "skipped"}; table: the learning rates.
    -> (families (None where absent), opt, record {"norm", "coef", "lr", "mask", "skipped": this step was})."""
    dt = np.float64 if f64 else F32
    table = np.asarray(table, np.float64 if f64 else F32).reshape(-1)
    part = [e is not None and int(e[2]) != 0 for e in fams]
    out = [None if e is None else dict(e[0]) for e in fams]
    if not any(part):
        return out, dict(opt), None
    with np.errstate(all="ignore"):
        gs = [None if not p else (np.asarray(e[1], dt) / dt(int(e[2]))).astype(dt) for e, p in zip(fams, part)]
        if f64:
            S = np.float64(sum(float(np.sum(g * g)) for g in gs if g is not None))
            norm = np.sqrt(S)
        else:
            S = sum_squares([g for g in gs if g is not None])
            norm = F32(np.sqrt(S))
        mx = dt(cfg["max_norm"])
        coef = dt(min(dt(1.0), dt(mx / dt(norm + dt(1e-6))))) if mx > 0 else dt(1.0)
        if mx > 0 and np.isnan(mx / dt(norm + dt(1e-6))):
            coef = dt(1.0)                           # fminf(1, NaN) = 1
        lr_t = table[min(int(opt["t"]), table.size - 1)]
        mask = sum(1 << k for k in range(3) if part[k])
        if cfg["skip_nonfinite"] and not np.isfinite(S):
            return out, {"t": opt["t"], "skipped": opt["skipped"] + 1}, {"norm": norm, "coef": dt(0.0), "lr": lr_t, "mask": mask, "skipped": True}
        b1, b2, eps, wd = dt(cfg["beta1"]), dt(cfg["beta2"]), dt(cfg["eps"]), dt(cfg["weight_decay"])
        omb1, omb2 = (dt(1.0) - b1, dt(1.0) - b2) if f64 else (_one_minus(b1), _one_minus(b2))
        for k in range(3):
            if not part[k]:
                continue
            st, g = out[k], gs[k]
            lr = dt(lr_t * dt(cfg["lr_scale"][k]))
            g = (g * coef).astype(dt)
            w = np.asarray(st["w"], dt)
            if wd > 0:
                if cfg["decoupled"]:
                    w = (w * dt(dt(1.0) - dt(lr * wd))).astype(dt)
                else:
                    g = (g + (wd * w).astype(dt)).astype(dt)
            m = (st["m"] + ((g - st["m"]).astype(dt) * omb1).astype(dt)).astype(dt)
            v = ((st["v"] * b2).astype(dt) + ((omb2 * g).astype(dt) * g).astype(dt)).astype(dt)
            bc1, bc2 = dt(dt(st["bc1"] * b1) + omb1), dt(dt(st["bc2"] * b2) + omb2)
            step_size = dt(lr / bc1)
            denom = ((np.sqrt(v).astype(dt) / np.sqrt(bc2).astype(dt)).astype(dt) + eps).astype(dt)
            w = (w - (step_size * (m / denom).astype(dt)).astype(dt)).astype(dt)
            out[k] = {"w": w, "m": m, "v": v, "t": st["t"] + 1, "bc1": bc1, "bc2": bc2}
    return out, {"t": opt["t"] + 1, "skipped": opt["skipped"]}, {"norm": norm, "coef": coef, "lr": lr_t, "mask": mask, "skipped": False}
