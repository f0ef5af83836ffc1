#!/usr/bin/env python3
"""Build libnpcd_hip.so for gfx950 with hipcc (cross-compiles without a GPU).

    python neural-point-cloud-diffusion_amd/csrc/build.py [--force]

Objects are rebuilt only when their source (or a header) is newer.  The library is written
in-tree to neural-point-cloud-diffusion_amd/lib/ so that it travels to the GPU box with the repo
snapshot (it is git-ignored, not gpurun-ignored).
"""
import concurrent.futures as cf
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_DIR = os.path.join(os.path.dirname(HERE), "lib")
OBJ_DIR = os.path.join(HERE, "build")
LIB = os.path.join(LIB_DIR, "libnpcd_hip.so")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
ARCH = "gfx950"

# source -> extra flags.  Geometry kernels must reproduce the oracle's fp32 operation order
# bit-exactly, so they are compiled without FMA contraction.
SOURCES = {
    "api.hip": [],
    # VGPR-form MFMA: accumulators stay in VGPRs (gfx950 has a unified register file), no v_accvgpr moves
    # -fno-honor-nans: no NaN can arise in the softmax math; drops the canonicalising v_max before every fmaxf
    # -fno-slp-vectorize: packed fp32 VALU (v_pk_mul/add_f32) is slower than two scalar ops beside MFMAs and
    # mis-pairs the 16-bit packing (MI355X_MICROARCH.md, per-instruction cycle constants)
    "attention.hip": ["-mllvm", "-amdgpu-mfma-vgpr-form", "-fno-honor-nans", "-fno-slp-vectorize"],
    "attention_gen.hip": ["-mllvm", "-amdgpu-mfma-vgpr-form", "-fno-honor-nans"],
    "geometry.hip": ["-ffp-contract=off"],
    "shade.hip": ["-mllvm", "-amdgpu-mfma-vgpr-form", "-fno-honor-nans"],
    # the rows kernel runs one wave per SIMD on the whole register file: accumulators (which the epilogues read) in VGPRs, the
    # activation fragments (matrix-instruction operands only) in AGPRs
    "shade_rows.hip": ["-mllvm", "-amdgpu-mfma-vgpr-form", "-fno-honor-nans"],
    "elementwise.hip": [],
    "sampler.hip": [],
    "gemm.hip": ["-mllvm", "-amdgpu-mfma-vgpr-form", "-fno-honor-nans"],
    "gemm_nt.hip": ["-mllvm", "-amdgpu-mfma-vgpr-form", "-fno-honor-nans"],
    "pairs.hip": ["-ffp-contract=off"],
    "pairs_mlp.hip": ["-mllvm", "-amdgpu-mfma-vgpr-form", "-fno-honor-nans"],
    "split.hip": [],
    "points_x2.hip": ["-mllvm", "-amdgpu-mfma-vgpr-form"],
    # the regularisers are compared with torch's fp32 operators term by term: evaluate the expressions as written
    "stage1_losses.hip": ["-ffp-contract=off"],
    # farthest point sampling picks by comparing fp32 squared distances bit for bit with its spec: no FMA contraction
    "fps.hip": ["-ffp-contract=off"],
    # the Chamfer kernel's per-point minima are the bits of its spec's fp32 distance expression, for the same reason.
    # -fno-slp-vectorize: its loop is nothing but fp32 VALU; packed into v_pk_mul/add_f32 (plus the moves that pair the operands) the
    # 2,000 x 512 self-matrix took 163 ms, as single operations 133 ms (docs/experiments.md R15.1)
    "chamfer.hip": ["-ffp-contract=off", "-fno-slp-vectorize"],
    # the approximate earth mover's distance evaluates the same fp32 distance expression as written; its sums are
    # explicit fused multiply-adds.  Single operations rather than packed ones, as for chamfer.hip
    "emd.hip": ["-ffp-contract=off", "-fno-slp-vectorize"],
    # the occupancy grid searches the valid cells with the same fp32 distance expression as written (clouds.h)
    "occupancy.hip": ["-ffp-contract=off"],
    # the image metrics evaluate their float64 expressions as written: with identical images the numerator and the denominator of
    # SSIM are then the same bits and the index is 1 exactly
    "ssim.hip": ["-ffp-contract=off"],
    # the feature statistics evaluate their float64 epilogues as written (cov from the raw moments, the cubic kernel): the exact-integer
    # tests and cov == cov.T rest on it; the products themselves are the float64 matrix instruction's
    "feature_stats.hip": ["-ffp-contract=off"],
    # the feature k-NN forms d2 = max((nx + ny) - 2 g, +0) and the squares of the norms as written: the exact-integer tests and "the same
    # bits for every split" rest on it
    "feature_manifold.hip": ["-ffp-contract=off"],
    # the isosurface's vertices are the bits of t = (level - f_lo) / (f_hi - f_lo) and origin + spacing * (i + t) as written: the
    # kernel is compared with its numpy restatement bit for bit
    "isosurface.hip": ["-ffp-contract=off"],
    # the vertex normals are the bits of their numpy restatement as well: gradient differences, the interpolation and the
    # normalisation as written
    "isosurface_normals.hip": ["-ffp-contract=off"],
    # the labelling is integer work; its one float operation is the isosurface's own inside test f > level
    "components.hip": ["-ffp-contract=off"],
    # surface sampling picks a face from integer weights floor(float64(d) 2^k) and places the point with (b0 v0 + b1 v1) + b2 v2: the
    # face measure d, the barycentric expressions and the normalisations are the bits of their numpy restatement only as written,
    # a fused multiply-add in the cross product would already move a weight
    "surface.hip": ["-ffp-contract=off"],
    # vertex clustering places a vertex in its cell and a cluster's representative by float64 expressions -- (u - c) 2^32 and
    # origin + cell (c + (S / n) 2^-32) -- that are the bits of their numpy restatement only as written: a fused multiply-add would
    # skip the rounding of a product
    "simplify.hip": ["-ffp-contract=off"],
    # a smoothing step moves a vertex by rint(f (S / d - q)) in float64, and the lattice is x 2^(29 - e) and back q 2^(e - 29): held
    # bit for bit to their numpy restatement, so every product, quotient and difference is rounded as written
    "smooth.hip": ["-ffp-contract=off"],
    # the closest face of a point is picked by comparing fp32 squared distances bit for bit with their numpy restatement: the six dot
    # products, the three cross terms and q = a + (v ab + w ac) are rounded as written.  Its pair loop is nothing
    # but fp32 VALU: single operations rather than packed ones, as for chamfer.hip (docs/experiments.md R15.1)
    "mesh_distance.hip": ["-ffp-contract=off", "-fno-slp-vectorize"],
    # the first hit of a ray is picked by comparing t = float(T / det) bit for bit with its numpy restatement: the fp32 shear of the
    # corners and the float64 edge functions, T and det are rounded as written.  Single operations, as above
    "raycast.hip": ["-ffp-contract=off", "-fno-slp-vectorize"],
    # the crossings of a ray are counted from the same corners, edge functions and t, compared bit for bit with their numpy
    # restatement: the flags of raycast.hip
    "crossings.hip": ["-ffp-contract=off", "-fno-slp-vectorize"],
}
COMMON = ["-O3", "-std=c++17", "-fPIC", f"--offload-arch={ARCH}", "-Wall", "-Wno-unused-function",
          "-fno-gpu-rdc", "-ffast-math" if False else "-fno-fast-math"]


def newer(a, b):
    return not os.path.exists(b) or os.path.getmtime(a) > os.path.getmtime(b)


def compile_one(src, extra, force):
    obj = os.path.join(OBJ_DIR, src.replace(".hip", ".o"))
    path = os.path.join(HERE, src)
    headers = [os.path.join(HERE, f) for f in os.listdir(HERE) if f.endswith(".h")]
    headers.append(os.path.join(os.path.dirname(os.path.dirname(HERE)), "include", "npcd_hip.h"))
    if force or newer(path, obj) or any(newer(h, obj) for h in headers):
        cmd = [HIPCC, *COMMON, *extra, *os.environ.get("NPCD_EXTRA_FLAGS", "").split(), "-c", path, "-o", obj]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"hipcc failed for {src}:\n{r.stdout}\n{r.stderr}")
        if r.stderr.strip():
            sys.stderr.write(r.stderr)
    return obj


def build(force=False, verbose=True):
    os.makedirs(LIB_DIR, exist_ok=True)
    os.makedirs(OBJ_DIR, exist_ok=True)
    srcs = {s: f for s, f in SOURCES.items() if os.path.exists(os.path.join(HERE, s))}
    with cf.ThreadPoolExecutor(max_workers=4) as ex:
        objs = list(ex.map(lambda kv: compile_one(kv[0], kv[1], force), srcs.items()))
    if force or any(newer(o, LIB) for o in objs):
        cmd = [HIPCC, "-shared", "-fPIC", f"--offload-arch={ARCH}", "-o", LIB, *objs]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"link failed:\n{r.stdout}\n{r.stderr}")
    if verbose:
        print(f"built {LIB} ({os.path.getsize(LIB) / 1024:.0f} KiB) from {sorted(srcs)}")
    return LIB


if __name__ == "__main__":
    build(force="--force" in sys.argv)
