"""Ablation builds of the single-pass chain kernel (tuning experiments only):
patches csrc/chain_tile.hip into build/var/chain_tile_abl.hip with one phase
removed per -D flag and links lib/libdspcore_<NAME>.so from it and the other
objects of the in-tree build.  Time them with tools/gpu_libs.sh.

    python tools/chain_ablation.py [NAME ...]   (default: all)

NOSRC   y = window samples (no SRC FMAs)     NOP1  no pass-1 sums (the float32
        input-normal sums; the float64 change of basis stays)
NOSCAN  no carry recurrences                       NOP2  no pass-2 cascade
NOYST   no y store                           NOZST no z store (also lets the
        compiler drop most of pass 2: read it together with NOP2)
NOSRC5  config 5's kernels (k_chain_gct/gcp): one add per output instead of the
        SRC's packed FMAs
"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dsp-audio-project_amd", "csrc")
BUILD = os.path.join(ROOT, "dsp-audio-project_amd", "build")
LIB = os.path.join(ROOT, "dsp-audio-project_amd", "lib")
HIPCC = "/opt/rocm/bin/hipcc"
FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-fno-slp-vectorize",
         f"-I{os.path.join(ROOT, 'include')}", f"-I{CSRC}"]
ALL = ["BASE", "NOSRC", "NOP1", "NOSCAN", "NOP2", "NOYST", "NOZST", "NOSRC5"]


def patched() -> tuple[str, str]:
    """(chain_tile.h, chain_tile.hip) with the ablation switches (round 6: the
    shared tile code moved to the header)."""
    SEP = "\n//@@SPLIT@@\n"
    s = open(os.path.join(CSRC, "chain_tile.h")).read() + SEP + \
        open(os.path.join(CSRC, "chain_tile.hip")).read()

    def rep(old, new, count=1):
        nonlocal s
        if s.count(old) != count:
            raise SystemExit(f"chain_tile.h/.hip changed; update the ablation patch near: {old[:60]!r}")
        s = s.replace(old, new)

    # SRC: y = window samples (k_chain_tile's DLY part of 48 and plain parts of 24)
    rep("    if constexpr (DLY) {\n      src_part<GEO, 0, 48, true>(xw, mt, y);",
        "#ifdef V_NOSRC\n#pragma unroll\n    for (int i = 0; i < TS; ++i) y[i] = xw[i];\n"
        "    if (false) {\n#else\n    if constexpr (DLY) {\n#endif\n      src_part<GEO, 0, 48, true>(xw, mt, y);")
    # pass 1 (float32 sums in input-normal coordinates): keep the change of
    # basis, drop the 6 v_pk_fma_f32 per sample
    rep("#pragma unroll\n    for (int j = 0; j < TS / 2; ++j) {",
        "#ifdef V_NOP1\n#pragma unroll\n    for (int d = 0; d < kD; ++d) e2[d] = f32x2{y[d], y[d + 1]};\n"
        "    if (false)\n#endif\n#pragma unroll\n    for (int j = 0; j < TS / 2; ++j) {")
    # carry (blocked scan): keep the LDS rows, drop the recurrences and the
    # segment Kogge-Stone (rows get E' as is)
    rep("  double u0 = e[0].x, u1 = e[0].y;\n", "  double u0 = e[0].x, u1 = e[0].y;\n#ifndef V_NOSCAN\n")
    rep("  // ---- 4. publish the tile's end state",
        "#else\n  for (int i = 0; i < 8; ++i)\n"
        "    *reinterpret_cast<f64x2*>(rows + (8 * sg + i + 1) * kScanRow + 2 * (kb < 6 ? kb : 6)) = e[i];\n"
        "#endif\n  // ---- 4. publish the tile's end state")
    rep("    store_tile<TS>(lds, y, lane, ry);\n",
        "#ifndef V_NOYST\n    store_tile<TS>(lds, y, lane, ry);\n#endif\n")
    rep("  {\n    double pend[kS];",
        "#ifdef V_NOP2\n  for (int t = 0; t < TS; ++t) y[t] = clip_f32(y[t] * g32 + (float)s1[t % kS], lo, hi);\n"
        "  if (false)\n#endif\n  {\n    double pend[kS];")
    rep("  store_tile<TS>(lds, y, lane_z, rz);",
        "#ifndef V_NOZST\n  store_tile<TS>(lds, y, lane_z, rz);\n#else\n"
        "  if (y[0] == 12345.f) a.z[0] = y[1];\n#endif")
    # config 5 (k_chain_gct / gcp): y = one window pair per output, no FMAs
    rep("          acc[o] = __builtin_elementwise_fma(t, X[g2 + pp], acc[o]);",
        "#ifdef V_NOSRC5\n          if (pp == 0) acc[o] = X[g2] + t;\n#else\n"
        "          acc[o] = __builtin_elementwise_fma(t, X[g2 + pp], acc[o]);\n#endif")
    hdr, hip = s.split(SEP)
    return hdr, hip


def main(names):
    os.makedirs(os.path.join(BUILD, "var"), exist_ok=True)
    import shutil
    src = os.path.join(BUILD, "var", "chain_tile_abl.hip")
    hdr, hip = patched()
    with open(os.path.join(BUILD, "var", "chain_tile.h"), "w") as f:
        f.write(hdr)
    with open(src, "w") as f:
        f.write(hip)
    # chain_pp.h and chain_plan.h next to the patched header, so that their
    # "chain_tile.h" is that one
    for h in ("chain_pp.h", "chain_plan.h"):
        shutil.copy(os.path.join(CSRC, h), os.path.join(BUILD, "var", h))
    others = [os.path.join(BUILD, f"{n}.o") for n in
              ("abi", "src_poly", "iir", "chain_plan", "chain_pp_0", "chain_pp_1", "chain_pp_2", "chain_pp_3",
               "fft", "fft_nf", "lfilter_nf", "audio_io")]
    procs = []
    for name in names:
        obj = os.path.join(BUILD, "var", f"chain_tile_{name}.o")
        d = [] if name == "BASE" else [f"-DV_{name}"]
        cmd = (f"{HIPCC} {' '.join(FLAGS + d)} -c {src} -o {obj} && "
               f"{HIPCC} --offload-arch=gfx950 -shared -fPIC -o {LIB}/libdspcore_{name}.so "
               f"{' '.join(others)} {obj}")
        procs.append((name, subprocess.Popen(cmd, shell=True)))
    for name, p in procs:
        if p.wait():
            raise SystemExit(f"build {name} failed")
        print("built", name)


if __name__ == "__main__":
    main(sys.argv[1:] or ALL)
