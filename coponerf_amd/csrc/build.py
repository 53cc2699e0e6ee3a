#!/usr/bin/env python
"""Build libcoponerf_hip.so for gfx950 with hipcc (cross-compiles without a GPU).

    python coponerf_amd/csrc/build.py [--force]

geometry.hip is compiled with -ffp-contract=off: its arithmetic must reproduce the oracle's
IEEE operation sequence bit for bit (sample coordinates / tap indices); ssim_warp.hip likewise, for the
sampling coordinates of the flow warp (its window sums name their FMAs), and summaries.hip, which shares them;
novel_views.hip for the one-rounding-per-operation sums of its resample and its byte pack; epipolar.hip for the float64
operation sequence of its fundamental matrices and line end points; point_cloud.hip for that of its points and votes; matches.hip
for the flow warp's fp32 sequence and the float64 sequence of its residuals, Jacobians and sums; splat.hip for the float64
sequence of its projection; ransac.hip for that of its 8-point systems, its residuals (sampson.h, shared with matches.hip, as
is pose_out.h: rel_pose's use and the pose written out), its split of the essential matrix (essential_split.h) and its polish,
which runs matches.hip's Gauss-Newton passes from pose_gauss_newton.h; ransac5.hip for that of its 5-point
solver, which tests/ransac5_ref.py follows bit for bit (both take their sampler and shape rule from ransac_common.h and their
system, elimination and null vectors from epipolar_system.h); ransac_h.hip for that of its homographies, their transfer errors
and their decomposition, which tests/homography_ref.py follows bit for bit (it shares ransac_score.h's tiling, jacobi_svd.h's
sweeps and ransac_common.h's winner with ransac.hip); model_select.hip for that of the homography's Sampson residual (sampson_h.h),
its Jacobians, sums and GRIC scores, which tests/model_select_ref.py follows (rotation_step.h and cholesky_solve.h are shared with matches.hip);
pose_eval.hip for that of its pose errors and of sampson.h's residual, whose bits its order statistics return (radix_select.h's
descent, shared with triangulate.hip); triangulate.hip for that of its pixel correction, its points and the depth ratios it ranks,
which tests/triangulate_ref.py follows bit for bit; bundle.hip for that of its residuals, Jacobians, Schur sums and covariances,
which tests/bundle_ref.py follows (it shares pose_gauss_newton.h's reduction and step with matches.hip and ransac.hip); mesh.hip
for that of its signed distances and vertices; raster.hip for that of its projection, depths and colours.  The last six share pinhole.h (the float64 camera; its bodies also switch contraction off by pragma) and
splat and raster zbuffer.h (the key, its atomic minimum, the resolve stores, the clear and the image checks).
"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(os.path.dirname(HERE), "libcoponerf_hip.so")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
COMMON = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function"]
UNITS = [
    ("error.cpp", []),
    ("streams.cpp", []),
    ("geometry.hip", ["-ffp-contract=off"]),
    ("gather.hip", []),
    ("encode.hip", []),
    ("encode_fused.hip", []),
    ("encode_f32.hip", []),
    ("guard.hip", []),
    ("local_units.hip", []),
    ("encode_bwd.hip", []),
    ("gemm_f16.hip", []),
    ("attend.hip", []),
    ("attend_units.hip", []),
    ("linear_f32.hip", []),
    ("rayout.hip", []),
    ("ufc_conv4d.hip", []),
    ("ufc_wgrad.hip", []),
    ("ufc_corr.hip", []),
    ("ufc_match.hip", []),
    ("ufc_attn.hip", []),
    ("ufc_strided_bwd.hip", []),
    ("encoder.hip", []),
    ("input.hip", []),
    ("backward.hip", []),
    ("wgrad_tall.hip", []),
    ("wgrad_f32.hip", []),
    ("adam.hip", []),
    ("trunk_conv.hip", []),
    ("pose.hip", []),
    ("ssim_warp.hip", ["-ffp-contract=off"]),
    ("image_metrics.hip", []),
    ("summaries.hip", ["-ffp-contract=off"]),
    ("lpips.hip", []),                                     # its two exact statements switch contraction off by pragma
    ("novel_views.hip", ["-ffp-contract=off"]),            # one rounding per operation in the resample sums and the byte pack
    ("epipolar.hip", ["-ffp-contract=off"]),               # one rounding per float64 operation of the line geometry
    ("point_cloud.hip", ["-ffp-contract=off"]),            # one rounding per float64 operation of the points and the votes
    ("matches.hip", ["-ffp-contract=off"]),                # flow_warp.h's fp32 sequence; float64 residuals, Jacobians and sums
    ("ransac.hip", ["-ffp-contract=off"]),                 # the float64 sequence of its systems, residuals and pose split
    ("ransac5.hip", ["-ffp-contract=off"]),                # the float64 sequence of the 5-point solver, bit for bit
    ("ransac_h.hip", ["-ffp-contract=off"]),               # the float64 sequence of the homography model, bit for bit
    ("model_select.hip", ["-ffp-contract=off"]),           # the float64 sequence of the homography's Sampson residual and GRIC
    ("pose_eval.hip", ["-ffp-contract=off"]),              # the float64 sequence of the pose errors and of sampson.h's residual
    ("triangulate.hip", ["-ffp-contract=off"]),            # the float64 sequence of the correction, the point and the ratios
    ("bundle.hip", ["-ffp-contract=off"]),                 # the float64 sequence of the residuals, the Schur sums and the covariances
    ("splat.hip", ["-ffp-contract=off"]),                  # one rounding per float64 operation of the projection
    ("mesh.hip", ["-ffp-contract=off"]),                   # one rounding per float64 operation of the TSDF and the vertices
    ("raster.hip", ["-ffp-contract=off"]),                 # one rounding per float64 operation of the projection and the depth
]


def _newer(src, dst):
    return (not os.path.exists(dst)) or os.path.getmtime(src) > os.path.getmtime(dst)


def build(force=False, verbose=True):
    objs = []
    # every header beside the sources, and the C interface: a changed header rebuilds every object
    deps = sorted(os.path.join(HERE, f) for f in os.listdir(HERE) if f.endswith(".h"))
    deps.append(os.path.join(HERE, "..", "..", "include", "coponerf_hip.h"))
    for name, extra in UNITS:
        src = os.path.join(HERE, name)
        obj = os.path.join(HERE, os.path.splitext(name)[0] + ".o")
        if force or _newer(src, obj) or any(_newer(d, obj) for d in deps):
            cmd = [HIPCC, *COMMON, *extra, "-x", "hip", "-c", src, "-o", obj]
            if verbose:
                print(" ".join(cmd), flush=True)
            subprocess.check_call(cmd)
        objs.append(obj)
    if force or any(_newer(o, OUT) for o in objs):
        cmd = [HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", *objs, "-o", OUT]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)
    return OUT


if __name__ == "__main__":
    print(build(force="--force" in sys.argv))
