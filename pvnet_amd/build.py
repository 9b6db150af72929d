"""Builds libpvnet_vote.so (the C-ABI HIP library) and the side libraries beside it (``SIDE_LIBRARIES``: one row per library, one
``libpvnet_<name>.so`` each) in-tree for gfx950 with hipcc.

    python -m pvnet_amd.build            # build if sources are newer than the library
    python -m pvnet_amd.build --force

hipcc cross-compiles without a GPU.  The library lands next to this file so that it travels with the tree."""
from __future__ import annotations

import os
import re
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(HERE, "csrc")
# one translation unit per stage (the map is at the top of vote_host.hip), then the pose solve after voting (pose_solve.hip) and
# the pose metrics after it (pose_metrics.hip);
# pvnet_rccl.hip is host code only: the RCCL binding
VOTE_TU = ["k1_mask.hip", "k2_compact.hip", "k3_hypotheses.hip", "k4_score_valu.hip", "k4_score_mfma.hip", "k4_score_exact.hip",
           "k4_score_cull.hip", "k5_refine.hip", "epilogues.hip", "pose_solve.hip", "pose_metrics.hip", "vote_host.hip"]
SRC = [os.path.join(CSRC, f) for f in VOTE_TU + ["pvnet_nn.hip", "pvnet_rccl.hip"]]
_POSE_CORE = os.path.join(CSRC, "pose_core.h")         # the one copy of the device pose solver: pose_solve.hip here and pose_classes.hip
DEPS = SRC + [os.path.join(CSRC, "vote_common.h"), os.path.join(CSRC, "k4_exact_body.h"), os.path.join(CSRC, "pvnet_rng.h"), _POSE_CORE,
              os.path.join(ROOT, "include", "pvnet_vote.h"), os.path.join(ROOT, "include", "pvnet_nn.h")]
LIB = os.path.join(HERE, "libpvnet_vote.so")          # release: the knobs are constants, the kernels the defaults reach
DEV_LIB = os.path.join(HERE, "libpvnet_vote_dev.so")  # -DPVNET_DEV: environment knobs + every kernel variant (knob tests, fuzz, tuning tools)
OBJ_DIR = os.path.join(HERE, "build")
ARCH = "gfx950"
# the head behind the backbone and the inputs in front of it: libraries of one translation unit each, beside libpvnet_vote.so, whose ABI
# stays as it is.  One row per library, under the name pvnet_amd._abi.SIDE_LIBRARIES binds it by:
# name -> (translation units, its header under include/, what they include beyond that header and the common ones)
_AUGMENT_WARP = os.path.join(CSRC, "augment_warp.h")   # the one copy of the plan and the warp: the two libraries that compile it rebuild with it
_MESH_CORE = os.path.join(CSRC, "mesh_core.h")         # the one copy of the projection and the coverage predicate, likewise
_ZBUFFER_CORE = os.path.join(CSRC, "zbuffer_core.h")   # the one copy of the z-buffer (it includes mesh_core.h and depth_core.h, the
                                                       # depth of a covered pixel): depth.hip, shade.hip and texture.hip
_PIXEL_COLOR = os.path.join(CSRC, "pixel_color.h")     # the one copy of the colour of a covered pixel: shade.hip and texture.hip
SIDE_LIBRARIES = {
    "head": (["head_metrics.hip"], "pvnet_head.h", []),          # the head metrics of a validation step
    "train": (["head_grad.hip"], "pvnet_train.h", []),           # the backward of the head losses of a training step
    "targets": (["head_targets.hip"], "pvnet_targets.h", []),    # the targets from key-points, the head fused with them
    "class_targets": (["class_targets.hip"], "pvnet_class_targets.h",   # the same from a label image and key-points per class
                      [os.path.join(ROOT, "include", "pvnet_targets.h"), os.path.join(ROOT, "include", "pvnet_classes.h")]),
    "augment": (["augment.hip"], "pvnet_augment.h", [_AUGMENT_WARP]),   # the inputs of a training step: warp, normalise, key-points
    "color": (["color_jitter.hip"], "pvnet_color.h",              # the colour jitter, alone or fused behind that warp
              [_AUGMENT_WARP, os.path.join(ROOT, "include", "pvnet_augment.h")]),
    "classes": (["class_split.hip"], "pvnet_classes.h", []),     # class labels -> the bit masks the voting layer runs on
    "raster": (["raster.hip"], "pvnet_raster.h", [_MESH_CORE]),     # poses and meshes -> silhouettes and label images
    "depth": (["depth.hip"], "pvnet_depth.h", [_ZBUFFER_CORE]),     # ... -> depth, occlusion-correct labels, visible pixel counts
    "shade": (["shade.hip"], "pvnet_shade.h", [_ZBUFFER_CORE, _PIXEL_COLOR]),       # ... -> shaded vertex-colour images over a background
    "poses": (["pose_classes.hip"], "pvnet_poses.h", [_POSE_CORE]),   # key-points per (image, class) -> a pose each, absent classes gated
    "trunk": (["trunk.hip"], "pvnet_trunk.h", []),               # a 3x3 conv of the residual trunk: BatchNorm, residual, activation fused
    "stem": (["stem.hip"], "pvnet_stem.h", []),                  # the network's stem in one launch: 7x7/2 conv, ReLU, 3x3/2 max-pool
    "decoder": (["decoder.hip"], "pvnet_decoder.h", []),         # a decoder stage in one launch: upsample, concat, 3x3 conv, LeakyReLU
    "tail": (["tail.hip"], "pvnet_tail.h", []),                  # the network's tail in one launch: upsample, concat, 3x3 and 1x1 conv
    "texture": (["texture.hip"], "pvnet_texture.h", [_ZBUFFER_CORE, _PIXEL_COLOR]),   # ... -> the same with UV-mapped textures
}


def _side(name):
    """(sources, what they depend on, the library) of one of SIDE_LIBRARIES.  The dependencies are the row's, closed under
    ``#include "..."`` of files in csrc/: a header that one of them includes rebuilds the library without being listed in its row."""
    tu, header, extra = SIDE_LIBRARIES[name]
    src = [os.path.join(CSRC, f) for f in tu]
    deps = src + [os.path.join(CSRC, f) for f in ("head_common.h", "vote_common.h", "pvnet_rng.h")] + \
        [os.path.join(ROOT, "include", f) for f in sorted({header, "pvnet_head.h", "pvnet_vote.h"})] + extra
    for d in deps:   # (grows while it is walked)
        if os.path.dirname(d) == CSRC and os.path.exists(d):
            with open(d) as fh:
                for inc in re.findall(r'^\s*#\s*include\s+"([^"]+)"', fh.read(), re.M):
                    path = os.path.join(CSRC, inc)
                    if os.path.exists(path) and path not in deps:
                        deps.append(path)
    return src, deps, os.path.join(HERE, f"libpvnet_{name}.so")


# host-side pose refinement (plain C++, g++): include/pvnet_pnp.h
PNP_SRC = os.path.join(HERE, "csrc", "pvnet_pnp.cpp")
PNP_DEPS = [PNP_SRC, os.path.join(ROOT, "include", "pvnet_pnp.h")]
PNP_LIB = os.path.join(HERE, "libpvnet_pnp.so")


def hipcc_path() -> str:
    for c in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return c
    raise RuntimeError("hipcc not found (set HIPCC or install ROCm under /opt/rocm)")


def flags():
    return ["-O3", "-std=c++17", f"--offload-arch={ARCH}", "-fPIC", "-shared", "-fno-fast-math",
            "-fno-slp-vectorize",  # keep the scoring loops as scalar v_sub/v_mul/v_fma (packed f32 gains nothing on gfx950)
            "-mllvm", "-amdgpu-mfma-vgpr-form",  # MFMA results straight into VGPRs: the vote's v_cmp reads them in place
            "-I", os.path.join(ROOT, "include"), "-I", os.path.join(HERE, "csrc"), "-Wall"]


def fresh(target, deps) -> bool:
    """the target exists and is no older than any of deps"""
    return os.path.exists(target) and all(os.path.getmtime(target) >= os.path.getmtime(d) for d in deps)


def up_to_date(lib=None) -> bool:
    return fresh(lib or LIB, DEPS)


def install(lib, make, check=None) -> None:
    """make(path) builds the library beside its place, check() judges the build, and only then does it replace the previous one: a
    failing compiler or check -- or a broken checker environment -- must not take a working library away"""
    tmp = lib + ".new"
    try:
        make(tmp)
        if check is not None:
            check()
        os.replace(tmp, lib)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)


def compile_link(out: str, dev: bool, verbose: bool = False) -> None:
    """every translation unit to an object file (in parallel: the exact-mode scoring kernels dominate), then one link"""
    from concurrent.futures import ThreadPoolExecutor
    os.makedirs(OBJ_DIR, exist_ok=True)
    cflags = [f for f in flags() if f != "-shared"] + (["-DPVNET_DEV"] if dev else [])
    objs = [os.path.join(OBJ_DIR, os.path.basename(src) + (".dev.o" if dev else ".o")) for src in SRC]

    def one(job):
        src, obj = job
        cmd = [hipcc_path()] + cflags + ["-c", src, "-o", obj]
        if verbose:
            print(" ".join(cmd))
        subprocess.check_call(cmd)

    # vote_host.hip last: pvnet_vote_build_info() reports how many kernels the library holds, counted in the other objects
    # (kernel descriptor symbols `<name>.kd` of their device code)
    jobs = [(src, obj) for src, obj in zip(SRC, objs) if not src.endswith("vote_host.hip")]
    with ThreadPoolExecutor(max_workers=min(len(jobs), 16, max(1, (os.cpu_count() or 4) - 1))) as ex:
        list(ex.map(one, jobs))
    names = set()
    for _, obj in jobs:
        names.update(re.findall(rb"[\w$.]+\.kd(?=\x00)", open(obj, "rb").read()))
    cflags.append(f"-DPVNET_KERNEL_COUNT={len(names)}")
    for src, obj in zip(SRC, objs):
        if src.endswith("vote_host.hip"):
            one((src, obj))
    cmd = [hipcc_path(), f"--offload-arch={ARCH}", "-shared", "-fPIC"] + objs + ["-o", out]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)


def build_pnp(force: bool = False, verbose: bool = False) -> str:
    if not force and fresh(PNP_LIB, PNP_DEPS):
        return PNP_LIB
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    if not cxx:
        raise RuntimeError("no C++ compiler found for libpvnet_pnp.so (set CXX)")
    cmd = [cxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread", "-Wall", "-I", os.path.join(ROOT, "include"), PNP_SRC,
           "-o", PNP_LIB]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    return PNP_LIB


def build_side(name: str, force: bool = False, verbose: bool = False) -> str:
    """hipcc -> one of SIDE_LIBRARIES, checked by the register tool for that library alone before it replaces the previous one"""
    src, deps, lib = _side(name)
    if force or not fresh(lib, deps):
        def make(out):
            cmd = [hipcc_path()] + flags() + src + ["-o", out]
            if verbose:
                print(" ".join(cmd))
            subprocess.check_call(cmd)

        install(lib, make, lambda: check_resources(("check_kernel_resources.py",), ["--" + name]))
    return lib


# the reference's compiled extension module `ransac_voting` (src/ransac_voting.cpp) on this library: host-only C++ against
# the torch headers, placed where the reference's driver imports it from
EXT_SRC = os.path.join(HERE, "csrc", "ransac_voting_ext.cpp")
EXT_DIR = os.path.join(ROOT, "lib", "ransac_voting_gpu_layer")


def ext_path() -> str:
    import sysconfig
    return os.path.join(EXT_DIR, "ransac_voting" + sysconfig.get_config_var("EXT_SUFFIX"))


def build_ext(force: bool = False, verbose: bool = False):
    """g++ -> lib/ransac_voting_gpu_layer/ransac_voting<EXT_SUFFIX> (linked against libpvnet_vote.so through an
    $ORIGIN-relative rpath).  Returns the path, or None when torch's headers / a C++ compiler are not available -- the
    pure-Python stand-in of the same name next to it serves the same four functions then."""
    import sysconfig
    out = ext_path()
    deps = [EXT_SRC, os.path.join(ROOT, "include", "pvnet_vote.h"), LIB]
    if not force and fresh(out, [d for d in deps if os.path.exists(d)]):
        return out
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    try:
        import torch
        from torch.utils import cpp_extension
    except Exception:
        return None
    if not cxx:
        return None
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    inc = cpp_extension.include_paths() + [os.path.join(rocm, "include"), os.path.join(ROOT, "include"),
                                           sysconfig.get_paths()["include"]]
    tlib = os.path.join(os.path.dirname(torch.__file__), "lib")
    cmd = [cxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-w", "-D__HIP_PLATFORM_AMD__=1", "-DUSE_ROCM=1",
           "-DTORCH_EXTENSION_NAME=ransac_voting", "-DTORCH_API_INCLUDE_EXTENSION_H",
           "-D_GLIBCXX_USE_CXX11_ABI=%d" % int(torch._C._GLIBCXX_USE_CXX11_ABI)]
    for i in inc:
        cmd += ["-I", i]
    cmd += [EXT_SRC, "-o", out, "-L", tlib, "-L", HERE, "-lc10", "-lc10_hip", "-ltorch", "-ltorch_cpu", "-ltorch_hip",
            "-ltorch_python", "-lpvnet_vote", "-Wl,-rpath," + tlib, "-Wl,-rpath,$ORIGIN/../../pvnet_amd"]
    if verbose:
        print(" ".join(cmd))
    try:
        subprocess.check_call(cmd)
    except (subprocess.CalledProcessError, OSError) as e:
        if os.path.exists(out):
            os.remove(out)
        print(f"pvnet_amd.build: the compiled ransac_voting module was not built ({e}); the Python stand-in serves it",
              file=sys.stderr)
        return None
    return out


# the compaction-flake canary (tests/test_flake_canary.py): the stand-alone reproducer of round 2's wrong-record flake, once as
# it failed (VGPR allocation used to its last granule) and once with the spare granule every kernel of the library keeps
CANARY_SRC = os.path.join(ROOT, "tools", "experiments", "k2_flake", "k2_repro.hip")
CANARY_BINS = {"tight": os.path.join(ROOT, "tools", "experiments", "k2_flake", "k2_repro_tight.bin"),
               "spare": os.path.join(ROOT, "tools", "experiments", "k2_flake", "k2_repro_spare.bin")}


def build_canary(force: bool = False, verbose: bool = False):
    for kind, out in CANARY_BINS.items():
        if not force and fresh(out, [CANARY_SRC]):
            continue
        cmd = [hipcc_path(), "-O3", f"--offload-arch={ARCH}", "-w", CANARY_SRC, "-o", out] + (["-DV_SPARE"] if kind == "spare" else [])
        if verbose:
            print(" ".join(cmd))
        subprocess.check_call(cmd)
    return CANARY_BINS


def check_resources(tools=("check_kernel_resources.py", "check_mfma_hazard.py"), args=()) -> None:
    """the spare-VGPR-granule rule is enforced AT BUILD TIME, not only by a CPU test that needs hipcc: a library
    whose kernels use their allocation to the last granule is not produced (tools/check_kernel_resources.py; the same for
    the hand-placed MFMA epilogues, tools/check_mfma_hazard.py).  The checkers compile the sources to assembly themselves;
    they run on the freshly built library's sources BEFORE it replaces the previous one (a failing check -- or a
    broken checker environment -- must not take a working library away).  PVNET_BUILD_UNCHECKED=1 skips them (experiments)."""
    if os.environ.get("PVNET_BUILD_UNCHECKED") == "1":
        print("pvnet_amd.build: PVNET_BUILD_UNCHECKED=1 -- register / MFMA-hazard checks SKIPPED (experiment build)", file=sys.stderr)
        return
    for tool in tools:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", tool)] + list(args), capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"pvnet_amd.build: tools/{tool} rejects this build (the previous library, if any, is kept):\n"
                               + r.stdout[-3000:] + r.stderr[-1000:])


def build(force: bool = False, verbose: bool = False) -> str:
    build_pnp(force, verbose)
    if force or not up_to_date(LIB):        # release: both checkers judge it
        install(LIB, lambda out: compile_link(out, dev=False, verbose=verbose), check_resources)
    if force or not up_to_date(DEV_LIB):    # development: not checked
        install(DEV_LIB, lambda out: compile_link(out, dev=True, verbose=verbose))
    for name in SIDE_LIBRARIES:
        build_side(name, force, verbose)
    build_ext(force, verbose)
    build_canary(force, verbose)
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
