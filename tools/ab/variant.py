"""Dev A/B (NOT product code): build a patched copy of the working-tree csrc into
tools/ab/libals_<tag>.so (same ABI, loaded with ALS_HIP_DEV=1 ALS_HIP_LIB=...).
Each variant is a list of (file, old, new) text replacements applied to the copy;
an `old` that does not occur fails the build (the patch must still apply).
    python tools/ab/variant.py TAG [TAG ...]      (TAG from VARIANTS below; "base" = none)
"""
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "..", "recommender-system-using-apache-spark-mllib-_amd", "csrc")
# headers of gram_solve.hip
GA, SC, SG, W1, DU = ("gram_accumulate.h", "solve_config.h", "solve_guards.h", "w1_solve.h",
                      "dual_solve.h")
TK = "topk_sweep.h"  # the top-k sweep kernel (topk.hip and topk_filtered.hip instantiate it)

VARIANTS = {
    "base": [],
    # top-k register lists: six blocks per ballot (logs keep four: their registers)
    "tk_nb6": [(TK, "constexpr int NB4 = 4;  // blocks per ballot",
                "constexpr int NB4 = (TOPR > 0 && TOPR <= 16) ? 6 : 4;  // blocks per ballot")],
    # the n x n dual kernel: step s+1's gathers in flight during step s at NB = 6 too
    "dualnb2": [(DU, "constexpr int NBUF = NB <= 4 ? 2 : 1;", "constexpr int NBUF = 2;")],
    # round 6: the LDL^T pivot-spread limit (rows beyond it go to the fp64 rescue)
    **{f"cond{c}": [(SC, "constexpr float kCondMax = 32.f;", f"constexpr float kCondMax = {c}.f;")]
       for c in (2, 4, 8, 16)},
    # occupancy: three waves per SIMD for the dual kernel
    "dual3": [
        (DU, "__launch_bounds__(64, 2) void gram_solve_dual_kernel(",
         "__launch_bounds__(64, 3) void gram_solve_dual_kernel("),
    ],
    # top-k timing bound (wrong scores by the hi.lo term): refinement without the lo
    # fetch (bl = 0), i.e. the cost of the lo loads' latency
    "tk_nolo": [
        (TK, """      __builtin_amdgcn_global_load_lds(Vlo + vr * RW + 4 * s + q, scr + s * 64, 16, 0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");""", """      (void)vr;"""),
        (TK, "const tk_half8 bl = __builtin_bit_cast(tk_half8, scr[s * 64 + lane]);",
         "const tk_half8 bl = {};"),
    ],
    # top-k logs (round 6) timing bound (no lists: wrong results): the sweep alone, every
    # quartet scored (V stream, LDS, MFMA, barriers), no block filtered
    "tk_sweeponly": [
        (TK, """            if (vb + 16 * (c + NB4) > n_v) {  // (uniform) the last tile""",
         """#pragma unroll
            for (int j = 0; j < NB4; ++j)
#pragma unroll
              for (int g = 0; g < RG; ++g)
                asm volatile("" :: "v"(a4[j][g][0]), "v"(a4[j][g][1]), "v"(a4[j][g][2]), "v"(a4[j][g][3]));
            if (true) continue;
            if (vb + 16 * (c + NB4) > n_v) {  // (uniform) the last tile"""),
    ],
    # timing bound (wrong results): the split-in-registers Gram (implicit) gathers only
    # rows 0..63 of Y (cache-hot): how much of the implicit launches is gather latency
    "hotgather": [
        (GA, "    TS::load_clamped(Y + (int64_t)(ids[j] >= 0 ? ids[j] : 0) * ld, s.y[j], d0, ld);",
         "    TS::load_clamped(Y + (int64_t)(ids[j] >= 0 ? (ids[j] & 63) : 0) * ld, s.y[j], d0, ld);"),
        (SG, "  if ((threadIdx.x & 63) == 0) {\n    const unsigned i = atomicAdd(rl.cnt, 1u);",
         "  if (false) {\n    const unsigned i = atomicAdd(rl.cnt, 1u);"),
    ],
    # top-k: 1.5x larger tiles at rank <= 64 (192 rows at k <= 64, 384 at k <= 32)
    "tk_vt_small": [
        (TK, "return topr == 0 ? 64 / nk : (nk == 4 ? 192 : 384 / nk);",
         "return topr == 0 ? 64 / nk : (nk == 4 ? 192 : 384 / nk);"),
    ],
    "tk_vt_small2": [
        (TK, "return topr == 0 ? 64 / nk : (nk == 4 ? 192 : 384 / nk);",
         "return topr == 0 ? 64 / nk : (nk == 4 ? 192 : 512 / nk);"),
    ],
    # the C-layout sweep only for NB = 4 (the round-4 choice) / in every elimination
    "sweepc_nb4": [
        (W1, "constexpr bool kSweepC = !SPLIT;", "constexpr bool kSweepC = NB == 4;"),
    ],
    "sweepc_all": [
        (W1, "constexpr bool kSweepC = !SPLIT;", "constexpr bool kSweepC = true;"),
    ],
}


def build(tag: str) -> str:
    # at the depth of csrc, so its "../../include" resolves to the repo's include/
    src = os.path.join(HERE, "..", "..", ".ab", tag)
    shutil.rmtree(src, ignore_errors=True)
    shutil.copytree(CSRC, src)
    for f, old, new in VARIANTS[tag]:
        p = os.path.join(src, f)
        s = open(p).read()
        if old not in s:
            raise SystemExit(f"{tag}: patch does not apply to {f}: {old[:70]!r}")
        open(p, "w").write(s.replace(old, new))
    objs = []
    procs = []
    for s in ("csr_build", "gram_solve", "predict", "topk", "topk_filtered"):
        o = os.path.join(src, s + ".o")
        objs.append(o)
        procs.append(subprocess.Popen(["/opt/rocm/bin/hipcc", "-O3", "-fPIC", "-std=c++17",
                                       "--offload-arch=gfx950", "-c", os.path.join(src, s + ".hip"),
                                       "-o", o]))
    for p in procs:
        if p.wait() != 0:
            raise SystemExit(f"{tag}: compile failed")
    lib = os.path.join(HERE, f"libals_{tag}.so")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-shared", "-fPIC", "--offload-arch=gfx950"] + objs
                          + ["-o", lib])
    if "--dev" in sys.argv:  # the phase-ablation kernels (tools/dev_ablate.hip) on this copy
        dev_src = os.path.join(src, "dev_ablate.hip")
        s = open(os.path.join(HERE, "..", "dev_ablate.hip")).read().replace(
            '"../recommender-system-using-apache-spark-mllib-_amd/csrc/gram_solve.hip"',
            '"gram_solve.hip"')
        open(dev_src, "w").write(s)
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-O3", "-fPIC", "-shared",
                               "--offload-arch=gfx950", "-std=c++17", dev_src, "-o",
                               os.path.join(HERE, f"libals_dev_{tag}.so")])
    shutil.rmtree(src)
    return lib


if __name__ == "__main__":
    for t in [a for a in sys.argv[1:] if not a.startswith("--")]:
        print("built", build(t), flush=True)
