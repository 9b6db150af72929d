"""Measures the pose solve per class (pnp.pnp_classes_device, voting.MultiPoseEvalWrapper) -> profiles/pose_classes_probe.txt.

    python tools/pose_classes_probe.py [--out FILE] [--rounds N] [--b B]          (needs an MI355X)

One MI355X, b = 32, pn = 9, nk = 3 and nk = 13 classes; float32 key-points (what the vote writes): the projections of every class's own
object points under a random pose, 0.4 px of noise (tests/pose_classes_cases.py's problems); every item present, and -- for nk = 13 -- with
8 of the 13 classes of every image marked absent in the vote's status.  Device events on one stream, the variants alternating, medians of
the rounds (each round: a window of 20 calls of every variant):
  (a) one ``pnp_classes_device`` call;
  (b) the loop it replaces: nk calls of ``pnp_batch_device`` on the class slices ``points_2d[:, k]`` with ``points_3d[k]`` (it cannot
      gate: absent classes are solved like the others);
  (c) ``pnp_batch_device`` on b nk items of ONE shared point set (as many problems, built the same way, every one a projection of
      class 0's points): the same number of waves through pose_solve_kernel, without the table and without the gate -- what the
      launch shape alone costs.  A wave's time is its LM iterations, so the mean iterations of (a) and (c) are printed beside them;
  (d) ``MultiPoseEvalWrapper`` whole (the per-class vote, then (a) gated by its status) against the same vote followed by (b), at
      480 x 640 and hn = 512 on tools/class_vote_probe.py's label images: three discs per image (classes 1, 2, 3), so that with
      nk = 13 ten classes of every image are absent.  The discs' key-points are no object's projections: the LM of a solved item runs long
      there (its mean iterations are printed), which is the same for both sides.
Also: the device assembly of pose_solve_kernel against the parent commit's (``--parent-asm FILE``: the parent's pose_solve.hip compiled
with ``build.flags()`` less ``-shared``, ``--cuda-device-only -S``), less the ``__hip_cuid_`` lines.  No threshold: the figures are
reported as they come.
"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from pvnet_amd import _abi, build, pnp as P, voting  # noqa: E402
from class_vote_probe import make_labels_and_field  # noqa: E402
from head_metrics_probe import H, W, VN  # noqa: E402
from tests import pose_classes_cases as CC  # noqa: E402

PN, HN, CALLS = 9, 512, 20


def device_asm(src):
    """the device assembly of one translation unit as the product's flags compile it, less the lines that name the compilation's id"""
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "k.s")
        subprocess.check_call([build.hipcc_path()] + [f for f in build.flags() if f != "-shared"] +
                              ["--cuda-device-only", "-S", "-Wno-unused-command-line-argument", src, "-o", out])
        return [line for line in open(out) if "__hip_cuid_" not in line]


def window_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(CALLS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / CALLS


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_classes_probe.txt"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--b", type=int, default=32)
    ap.add_argument("--parent-asm", default=None, help="device assembly of the parent commit's pose_solve.hip (see above)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the probe needs the GPU: nothing here is measured without one"
    dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    b = args.b
    say(f"pose_classes_probe: {torch.cuda.get_device_name(0)}, b={b}, pn={PN}, float32 key-points, 0.4 px noise; times are means of "
        f"device-event windows of {CALLS} calls, median over {args.rounds} alternating rounds (min..max)")
    if args.parent_asm:
        ours = device_asm(os.path.join(build.CSRC, "pose_solve.hip"))
        parent = [line for line in open(args.parent_asm) if "__hip_cuid_" not in line]
        say(f"pose_solve_kernel: device assembly of pose_solve.hip (flags() less -shared, --cuda-device-only -S, less the __hip_cuid_ "
            f"lines) against the parent commit's: {len(ours)} lines against {len(parent)}, "
            f"{'IDENTICAL line for line' if ours == parent else 'DIFFERENT'}")

    def measure(variants):
        for _, fn in variants:
            window_ms(fn)
        t = {n: [] for n, _ in variants}
        for _ in range(args.rounds):
            for n, fn in variants:
                t[n].append(window_ms(fn))
        for n, _ in variants:
            v = t[n]
            say(f"  {n:64s} {sorted(v)[len(v) // 2] * 1e3:9.1f} us  ({min(v) * 1e3:.1f} .. {max(v) * 1e3:.1f})")
        return {n: (sorted(v)[len(v) // 2], max(v) - min(v)) for n, v in t.items()}

    Kd = torch.from_numpy(P.LINEMOD_K.copy()).to(dev)
    for nk in (3, 13):
        X, x2, _ = CC.case(b, nk, PN, noise=CC.NOISE)
        Xd = torch.from_numpy(X).to(dev)
        pts = torch.from_numpy(x2.astype(np.float32)).to(dev)
        # (c)'s items: as many, built the same way, but every one a projection of ONE point set (class 0's)
        Xc, x2c, _ = CC.case(b * nk, 1, PN, noise=CC.NOISE)
        Xc, flat = torch.from_numpy(Xc[0]).to(dev), torch.from_numpy(x2c[:, 0].astype(np.float32)).to(dev)
        poses = torch.empty((b, nk, 3, 4), dtype=torch.float64, device=dev)
        status = torch.empty((b, nk), dtype=torch.int32, device=dev)
        poses1 = torch.empty((b, 3, 4), dtype=torch.float64, device=dev)
        status1 = torch.empty((b,), dtype=torch.int32, device=dev)
        posesc = torch.empty((b * nk, 3, 4), dtype=torch.float64, device=dev)
        statusc = torch.empty((b * nk,), dtype=torch.int32, device=dev)
        slices = [pts[:, k] for k in range(nk)]

        def path_a(vs=None):
            P.pnp_classes_device(Xd, pts, Kd, vote_status=vs, out=(poses, status))

        def path_b():
            for k in range(nk):
                P.pnp_batch_device(Xd[k], slices[k], Kd, out=(poses1, status1))

        def path_c():
            P.pnp_batch_device(Xc, flat, Kd, out=(posesc, statusc))

        say()
        say(f"== nk = {nk}: {b * nk} items, every item present")
        variants = [("(a) pnp_classes_device, one launch", path_a), (f"(b) {nk} x pnp_batch_device on class slices", path_b),
                    (f"(c) pnp_batch_device on {b * nk} items, one shared point set", path_c)]
        m = measure(variants)
        (ta, _), (tb, sb) = m[variants[0][0]], m[variants[1][0]]
        say(f"  (a) / (b) = {ta / tb:.3f};  (b)'s spread {sb * 1e3:.1f} us;  (a) below (b) by more than that spread: {tb - ta > sb};  "
            f"(a) / (c) = {ta / m[variants[2][0]][0]:.3f};  mean LM iterations (a) {status.float().mean().item():.1f}, (c) {statusc.float().mean().item():.1f}")
        if nk == 13:
            gen = torch.Generator().manual_seed(3)
            absent = torch.stack([torch.randperm(nk, generator=gen) < 8 for _ in range(b)])    # 8 of the 13 classes of every image
            vs = (absent[:, :, None] * _abi.S_SKIPPED).expand(b, nk, PN).to(torch.int32).contiguous().to(dev)
            say(f"== nk = {nk}: {b * nk} items, 8 of 13 classes of every image absent in the vote's status ({int(absent.sum())} items); "
                f"(b) and (c) cannot gate and are the rows above")
            g = measure([("(a) pnp_classes_device, one launch, gated", lambda: path_a(vs))])
            ta = g["(a) pnp_classes_device, one launch, gated"][0]
            say(f"  (a) / (b) = {ta / tb:.3f};  (a) below (b) by more than (b)'s spread: {tb - ta > sb}")

    # (d) the whole step behind the backbone
    labels, vertex = make_labels_and_field(b, dev, 500)
    field = vertex.view(b, H, W, 2 * VN).permute(0, 3, 1, 2)    # the backbone's layout, a view of the same memory
    for nk in (3, 13):
        X = CC.class_points(nk, VN)
        wrap = voting.MultiPoseEvalWrapper(X, P.LINEMOD_K, round_hyp_num=HN)
        Xd = torch.from_numpy(X).to(dev)
        ws = torch.empty(voting.vote_layout(b * nk, H, W, VN, HN, 30000).total_bytes, dtype=torch.uint8, device=dev)
        kp = torch.empty((b, nk, VN, 2), device=dev)
        poses = torch.empty((b, nk, 3, 4), dtype=torch.float64, device=dev)
        status = torch.empty((b, nk), dtype=torch.int32, device=dev)
        poses1 = torch.empty((b, 3, 4), dtype=torch.float64, device=dev)
        status1 = torch.empty((b,), dtype=torch.int32, device=dev)

        def whole():
            wrap(labels, field, use_argmax=False, seed=3, workspace=ws, kpts_out=kp, out=(poses, status))

        def vote_then_loop():
            voting.ransac_voting_layer_v2(labels, vertex, nk + 1, HN, inlier_thresh=0.99, seed=3, return_status=True, workspace=ws, out=kp)
            for k in range(nk):
                P.pnp_batch_device(Xd[k], kp[:, k], Kd, out=(poses1, status1))

        def vote_alone():
            voting.ransac_voting_layer_v2(labels, vertex, nk + 1, HN, inlier_thresh=0.99, seed=3, return_status=True, workspace=ws, out=kp)

        say()
        whole()
        torch.cuda.synchronize()
        say(f"== (d) nk = {nk}, {H}x{W}, hn = {HN}, three discs per image: {int((status == P.POSE_ABSENT).sum())} of {b * nk} items absent, "
            f"{int((status >= 0).sum())} solved, their mean LM iterations {status[status >= 0].float().mean().item():.1f}")
        variants = [("(d) MultiPoseEvalWrapper whole", whole), (f"    the vote, then {nk} x pnp_batch_device", vote_then_loop),
                    ("    the vote alone", vote_alone)]
        m = measure(variants)
        (tw, _), (tl, sl) = m[variants[0][0]], m[variants[1][0]]
        say(f"  whole / (vote, then loop) = {tw / tl:.3f};  the loop's spread {sl * 1e3:.1f} us;  below it by more than that spread: {tl - tw > sl}")
        del ws
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
