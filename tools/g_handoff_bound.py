#!/usr/bin/env python3
"""Upper bound of an on-chip hand-off of the gate matrix G: a TIMING-ONLY build from patched COPIES
of csrc (build/g_bound/, never the shipped sources) in which, from a context's third classify call on and under the named switches,
  UVAD_EXP_NOSTORE=1  the weight-stationary projection issues no store of its finished tile (everything else of the kernel runs: operand
                      stream, MFMAs, staging of the tile in LDS, the piece reads), and
  UVAD_EXP_L2STORE=1  ... or issues every store, but over the workgroup's first tile (64 KB rewritten again and again: the stores land in L2), and
  UVAD_EXP_NOREAD=1   the 16-sequence recurrence takes its gate rows from the first 8 frames of its sequences over and over (2 MB per launch,
                      L2-resident) instead of streaming the 1.05 GB of G from HBM.
The first two calls of every context run unpatched, so G holds the finite gate values of a real projection for the rest of the run and the
recurrences see realistic operands (matrix instructions on NaN or constant operands draw less power, and this regime runs at the power cap:
DESIGN.md 5b-2).  NOSTORE + NOREAD = a hand-off that costs nothing: what no producer / consumer kernel can beat; L2STORE + NOREAD = a hand-off through an
L2-resident ring with free synchronisation (the producer still issues its stores).  Logits of these runs are
wrong by construction; only the step time is read (bench.py's in-flight identity check is expected to fail).
    python tools/g_handoff_bound.py build     # here: build/g_bound/libuvad_gbound.so
    python tools/g_handoff_bound.py run       # on the GPU box: the 200-step in-flight bench for the four switch settings, alternating"""
import json, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "universal-voice-activity-detection_amd", "csrc")
OUT = os.path.join(ROOT, "build", "g_bound")
FLAGS = {"gemm_f16p_ws": ["-mllvm", "-amdgpu-mfma-vgpr-form=1", "-fno-slp-vectorize"], "lstm": ["-mllvm", "-amdgpu-mfma-vgpr-form=1", "-fno-slp-vectorize"], "uvad_api": []}


def sub(src, a, b, count=1):
    assert src.count(a) == count, (src.count(a), a[:80])
    return src.replace(a, b)


def patched(name):
    src = open(os.path.join(CSRC, name + ".hip")).read()
    if name == "gemm_f16p_ws":   # GemmArgs::B (unused by this kernel) == -7: no store instruction
        src = sub(src, "        __builtin_nontemporal_store(pc[piece_begin<NKB>(kb - 1) + (t_)], reinterpret_cast<f32x4 *>(gprev + (size_t)(piece_begin<NKB>(kb - 1) + (t_)) * (8 * 64)));",
                  "        { if (a.B != -7) __builtin_nontemporal_store(pc[piece_begin<NKB>(kb - 1) + (t_)], reinterpret_cast<f32x4 *>(gprev + (size_t)(piece_begin<NKB>(kb - 1) + (t_)) * (8 * 64))); }")
        src = sub(src, "        __builtin_nontemporal_store(o, reinterpret_cast<f32x4 *>(gprev + (size_t)p * (8 * 64)));",
                  "        if (a.B != -7) __builtin_nontemporal_store(o, reinterpret_cast<f32x4 *>(gprev + (size_t)p * (8 * 64)));")
        # GemmArgs::B == -8: every finished tile is stored over the workgroup's FIRST tile (64 KB per workgroup, rewritten again and again: the stores
        # are issued in full but land in L2) -- what a hand-off through an L2-resident ring would still pay on the producer's side
        src = sub(src, "        float *gout = a.C + ((size_t)r_cur * n64 + g_ntile) * (128 * 64) + g_lane;",
                  "        float *gout = a.C + ((size_t)(a.B == -8 ? r_first : r_cur) * n64 + g_ntile) * (128 * 64) + g_lane;")
        src = sub(src, "    int r_cur = __builtin_amdgcn_readfirstlane(rowtile(c_cur));",
                  "    int r_cur = __builtin_amdgcn_readfirstlane(rowtile(c_cur));\n    const int r_first = r_cur;")
    if name == "lstm":           # LstmArgs::t_begin[0] (unused by the 16-sequence kernel) == -7: the gate rows of frames 0 .. 7, again and again
        src = sub(src, "        if (s + 1 < a.T) advance(g_p, g_rl, g_in, g_wrap);   // the gates of the next step (the last step re-reads its own)",
                  "        if (a.t_begin[0] == -7) { if ((s & 7) == 7) { g_p = g_p0; g_rl = g_rl0; } else advance(g_p, g_rl, g_in, g_wrap); }\n"
                  "        else if (s + 1 < a.T) advance(g_p, g_rl, g_in, g_wrap);")
        src = sub(src, "    float c[RB];\n#pragma unroll\n    for (int rb = 0; rb < RB; ++rb) c[rb] = 0.0f;\n    f32x4 gq[RB];",
                  "    const float *const g_p0 = g_p; const int g_rl0 = g_rl;\n    float c[RB];\n#pragma unroll\n    for (int rb = 0; rb < RB; ++rb) c[rb] = 0.0f;\n    f32x4 gq[RB];")
        # the launcher refuses steps > 0 only; t_begin is not looked at for steps == 0
    if name == "uvad_api":
        src = sub(src, "            if (mode_is_ws(c) && gemm_f16p_ws_supported(g, c->n_cu))   // large launches: weights stay in registers, bit-identical gates",
                  "            if (exp_on && getenv(\"UVAD_EXP_NOSTORE\")) g.B = -7;\n            if (exp_on && getenv(\"UVAD_EXP_L2STORE\")) g.B = -8;\n"
                  "            if (mode_is_ws(c) && gemm_f16p_ws_supported(g, c->n_cu))   // large launches: weights stay in registers, bit-identical gates")
        src = sub(src, "        r.products = f16 ? mode_products(c) : 4;\n        if (ss) {",
                  "        r.products = f16 ? mode_products(c) : 4;\n        if (exp_on && getenv(\"UVAD_EXP_NOREAD\")) r.t_begin[0] = -7;\n        if (ss) {")
        src = sub(src, "    const uvad_model_cfg &m = c->mc;\n    const WsLayout w = carve(c, B, T);\n    if (ws_bytes < w.total) return fail(c, UVAD_E_WORKSPACE,",
                  "    const uvad_model_cfg &m = c->mc;\n    static std::map<uvad_ctx *, int> exp_calls;\n    const bool exp_on = ++exp_calls[c] > 2;\n"
                  "    const WsLayout w = carve(c, B, T);\n    if (ws_bytes < w.total) return fail(c, UVAD_E_WORKSPACE,")
        if "#include <cstdlib>" not in src:
            src = "#include <cstdlib>\n" + src
    return src


def build():
    os.makedirs(OUT, exist_ok=True)
    objs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".o") and f[:-2] not in FLAGS]
    for name, fl in FLAGS.items():
        p = os.path.join(OUT, name + ".hip")
        open(p, "w").write(patched(name))
        o = p[:-4] + ".o"
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-fast-math", "-Wno-unused-function"] + fl +
                              [f"-I{CSRC}", f"-I{os.path.join(ROOT, 'include')}", "-c", p, "-o", o])
        objs.append(o)
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-shared", "-fPIC", "-o", os.path.join(OUT, "libuvad_gbound.so")] + objs)
    print("built", os.path.join(OUT, "libuvad_gbound.so"))


def run():
    lib = os.path.join(OUT, "libuvad_gbound.so")
    settings = [("as_shipped", {}), ("no_store", {"UVAD_EXP_NOSTORE": "1"}), ("no_read", {"UVAD_EXP_NOREAD": "1"}),
                ("no_store_no_read", {"UVAD_EXP_NOSTORE": "1", "UVAD_EXP_NOREAD": "1"}),
                ("l2_store_no_read", {"UVAD_EXP_L2STORE": "1", "UVAD_EXP_NOREAD": "1"})]
    res = {k: [] for k, _ in settings}
    for rep in range(2):          # alternating: the boxes' clocks drift
        for name, env in settings:
            e = dict(os.environ, **env)
            p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bench_lib.py"), lib, "--steps", "200", "--warmup", "3", "--full", "--no-cpu-baseline", "--no-sincnet",
                                "--no-sequential", "--no-reference-shape"], env=e, capture_output=True, text=True, timeout=600)
            line = [l for l in p.stdout.splitlines() if l.startswith("{")]
            if not line:
                print(json.dumps({"setting": name, "error": p.stderr[-300:]}), flush=True)
                continue
            d = json.loads(line[-1])
            alone = d["roofline"]["alone_on_gpu"]
            res[name].append(d["value"])
            print(json.dumps({"setting": name, "rep": rep, "frames_per_s": d["value"], "ms_per_step": d["ms_per_step"], "outputs_identical": d["in_flight_outputs_identical_to_single_call"],
                              "alone_on_gpu_ms": {k: alone[k] for k in ("proj_k256_ms", "proj_layer0_ms", "recurrent_launch_ms", "step_ms")},
                              "sclk_mhz": (d.get("clocks_during_timed_region") or {}).get("sclk_mhz", {}).get("median")}), flush=True)
    base = sum(res["as_shipped"]) / max(len(res["as_shipped"]), 1)
    print(json.dumps({"summary": {k: {"mean_frames_per_s": sum(v) / len(v), "vs_as_shipped": sum(v) / len(v) / base} for k, v in res.items() if v}}), flush=True)


if __name__ == "__main__":
    {"build": build, "run": run}[sys.argv[1]]()
