"""Measures the targets of several objects on the GPU (pvnet_amd/validation.py: vertex_targets_classes_device,
HeadLoss.from_class_keypoints) and compares the code generated for libpvnet_targets.so with another tree's
-> profiles/class_targets_probe.txt (two sections; a run rewrites its own and keeps the other).

    python tools/class_targets_probe.py [--out FILE] [--rounds N] [--b B]      # the measurement: needs the GPU
    python tools/class_targets_probe.py --codegen OTHER_TREE [--out FILE]      # the comparison: needs hipcc only

Measurement: one MI355X, b = 32, 480 x 640, vn = 9, int64 labels, float32 and bfloat16 predictions; class_num = 4 and 14 on the
class-vote probe's three-disc labels (tools/class_vote_probe.py: with 14 classes ten are absent) and on vertical stripes of period 3
through all the classes, the worst case for the lookup -- nearly every lane's eight pixels hold three classes.  Two input sets are
cycled, device events on one stream, the variants alternating, medians of the rounds:
  (a) ``HeadLoss.from_class_keypoints`` forward + backward of mean(loss_seg) + 0.5 mean(loss_vertex);
  (b) what it replaces: class_num - 1 calls of ``vertex_targets_device`` on ``labels == k + 1`` (building each mask included), the
      adds into one field and one plane of weights, and ``HeadLoss`` forward + backward on them;
  (c) ``HeadLoss.from_keypoints`` on the binary mask ``labels > 0`` of the same foreground with one class's key-points: the
      single-class fused cost, so (a) - (c) is what the lookup by label costs;
  (d) ``vertex_targets_classes_device`` alone against ONE ``vertex_targets_device`` call alone (on that binary mask);
  (e) a device copy that moves as many bytes as (a) reads and writes.
The gradients of (a) and (b) are compared with torch.equal before anything is timed.  No threshold: the figures are reported as
they come.

Comparison: head_targets.hip of this tree and of OTHER_TREE compiled to assembly with the product's flags; per kernel the
instruction stream and the descriptor (tools/check_kernel_resources.kernel_code), and the files line for line but the
compilation-unit id, which is a hash of the source text.
"""
import argparse
import difflib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

SECTIONS = ("== codegen", "== measurement")


def write_section(path, which, lines):
    """replace the section that starts with SECTIONS[which] in the file (or add it), keep the other"""
    parts = {0: [], 1: []}
    if os.path.exists(path):
        cur = None
        for line in open(path).read().splitlines():
            for k, head in enumerate(SECTIONS):
                if line.startswith(head):
                    cur = k
            if cur is not None:
                parts[cur].append(line)
    parts[which] = lines
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(parts[0] + ([""] if parts[0] and parts[1] else []) + parts[1]) + "\n")


def codegen(other, out):
    import check_kernel_resources as chk
    from pvnet_amd import build as B
    lines = [f"{SECTIONS[0]}: head_targets.hip (libpvnet_targets.so), this tree against the tree before kp_target moved into kp_target.h =="]
    asm = []
    with tempfile.TemporaryDirectory() as d:
        for k, tree in enumerate((other, ROOT)):
            flags = [f.replace(ROOT, tree) if f.startswith(ROOT) else f for f in B.flags() if f not in ("-shared", "-fPIC")]
            dst = os.path.join(d, f"t{k}.s")
            subprocess.check_call([B.hipcc_path()] + flags + ["-S", "--cuda-device-only", "-Wno-unused-command-line-argument",
                                                              os.path.join(tree, "pvnet_amd", "csrc", "head_targets.hip"), "-o", dst],
                                  stderr=subprocess.DEVNULL)
            asm.append(open(dst).read())
    cuid = re.compile(r"__hip_cuid_[0-9a-f]+")
    a, b = ([cuid.sub("__hip_cuid_X", line) for line in t.splitlines()] for t in asm)
    delta = [line for line in difflib.unified_diff(a, b, lineterm="", n=0) if not line.startswith(("---", "+++", "@@"))]
    ka, kb = chk.kernel_code(asm[0]), chk.kernel_code(asm[1])
    differ = sorted(n for n in set(ka) | set(kb) if ka.get(n) != kb.get(n))
    lines.append(f"  kernels: {len(ka)} before, {len(kb)} now; instruction stream or descriptor differs in {len(differ)}"
                 + ("" if not differ else ": " + ", ".join(chk.short(n) for n in differ)))
    lines.append(f"  assembly files: {len(a)} lines before, {len(b)} now; lines that differ, the compilation-unit id (a hash of the source "
                 f"text) aside: {len(delta)}")
    lines += ["    " + line for line in delta[:40]]
    lines.append("  device assembly of libpvnet_targets.so is the parent's line for line: " + ("yes" if not delta and not differ else "NO"))
    # the new library's kernels beside the single-class ones: allocation and occupancy
    new = {chk.short(n): (nfv, s) for _, t in chk.side_assembly("class_targets") for n, nfv, _, s in chk.kernels(t)}
    old = {chk.short(n): (nfv, s) for n, nfv, _, s in chk.kernels(asm[1])}
    lines.append("  VGPRs allocated (waves per SIMD), scratch bytes: class_targets.hip against the same kernel of head_targets.hip")
    pairs = (("vertex_targets_classes_kernelILb1", "vertex_targets_kernelILb1"), ("head_partial_ckp_kernelILi0ELi1", "head_partial_kp_kernelILi0ELi1"),
             ("head_partial_ckp_kernelILi2ELi1", "head_partial_kp_kernelILi2ELi1"), ("head_grad_ckp_kernelILi0ELi1", "head_grad_kp_kernelILi0ELi1"),
             ("head_grad_ckp_kernelILi2ELi1", "head_grad_kp_kernelILi2ELi1"), ("head_partial_ckp_general", "head_partial_kp_general"),
             ("head_grad_ckp_general", "head_grad_kp_general"))
    for pn, po in pairs:
        (n1, (v1, s1)), = [(n, v) for n, v in new.items() if n.startswith(pn)]
        (n0, (v0, s0)), = [(n, v) for n, v in old.items() if n.startswith(po)]
        al1, al0 = (v1 + 7) // 8 * 8, (v0 + 7) // 8 * 8
        lines.append(f"    {pn:36s} {al1:3d} ({min(8, 512 // al1)}), {s1} B    {po:32s} {al0:3d} ({min(8, 512 // al0)}), {s0} B")
    for line in lines:
        print(line)
    write_section(out, 0, lines)


def measure(args):
    import torch
    from pvnet_amd import validation as V
    from head_metrics_probe import H, W, VN, time_ms
    from class_vote_probe import make_labels_and_field
    assert torch.cuda.is_available(), "the probe needs the GPU: nothing here is measured without one"
    dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    b = args.b
    say(f"{SECTIONS[1]}: {torch.cuda.get_device_name(0)}, b={b}, {H}x{W}, vn={VN}, int64 labels, sigma=1; times are means of device-event "
        f"windows, median over {args.rounds} alternating rounds (min..max) ==")
    loss = V.HeadLoss()
    xs = torch.arange(W, device=dev)[None, None, :]
    verdicts = []
    for dtype, name in ((torch.float32, "float32"), (torch.bfloat16, "bfloat16")):
        esz = 2 if dtype == torch.bfloat16 else 4
        for class_num in (4, 14):
            nk = class_num - 1
            planes = class_num + 2 * VN
            moved = b * H * W * (2 * (planes * esz + 8) + planes * esz)   # forward reads + backward reads, gradients written
            for kind in ("three discs", "stripes of period 3"):
                sets = []
                for k in range(2):
                    g = torch.Generator(device=dev).manual_seed(100 * class_num + k)
                    if kind == "three discs":
                        labels, _ = make_labels_and_field(b, dev, 7 + k)
                    else:
                        labels = ((xs // 3 + 1 + torch.arange(b, device=dev)[:, None, None]) % class_num).expand(b, H, W).contiguous()
                    hc = torch.cat([torch.rand((b, nk, VN, 1), generator=g, device=dev, dtype=torch.float64) * W,
                                    torch.rand((b, nk, VN, 1), generator=g, device=dev, dtype=torch.float64) * H,
                                    torch.ones((b, nk, VN, 1), device=dev, dtype=torch.float64)], 3)
                    seg = torch.randn((b, class_num, H, W), generator=g, device=dev).to(dtype).requires_grad_(True)
                    vp = torch.randn((b, 2 * VN, H, W), generator=g, device=dev).to(dtype).requires_grad_(True)
                    sets.append((seg, vp, labels, hc, (labels > 0).to(torch.int64), hc[:, 0].contiguous()))
                field = torch.empty((b, 2 * VN, H, W), device=dev)
                weights = torch.empty((b, 1, H, W), device=dev)
                tmp = (torch.empty_like(field), torch.empty_like(weights))
                half = torch.empty(moved // 2, dtype=torch.uint8, device=dev)
                half2 = torch.empty_like(half)

                def step(ls, lv, s):
                    s[0].grad = s[1].grad = None
                    (ls.mean() + 0.5 * lv.mean()).backward()

                def path_a(s):
                    ls, lv, _, _ = loss.from_class_keypoints(s[0], s[1], s[2], s[3])
                    step(ls, lv, s)

                def path_b(s):
                    field.zero_()
                    weights.zero_()
                    for c in range(nk):
                        V.vertex_targets_device((s[2] == c + 1).to(torch.uint8), s[3][:, c], out=tmp)
                        field.add_(tmp[0])
                        weights.add_(tmp[1])
                    ls, lv, _, _ = loss(s[0], s[1], s[2], field, weights)
                    step(ls, lv, s)

                def path_c(s):
                    # (the logits keep their class_num planes: the binary mask's labels 0 / 1 are labels of theirs)
                    ls, lv, _, _ = loss.from_keypoints(s[0], s[1], s[4], s[5])
                    step(ls, lv, s)

                variants = [("(a) HeadLoss.from_class_keypoints fwd+bwd", path_a),
                            (f"(b) {nk} x vertex_targets_device, adds, HeadLoss", path_b),
                            ("(c) HeadLoss.from_keypoints, binary mask", path_c),
                            ("(d) vertex_targets_classes_device alone", lambda s: V.vertex_targets_classes_device(s[2], s[3], out=tmp)),
                            ("(d) one vertex_targets_device alone", lambda s: V.vertex_targets_device(s[4], s[5], out=tmp)),
                            ("(e) a device copy of (a)'s bytes", lambda s: half2.copy_(half))]
                path_a(sets[0])
                ga = (sets[0][0].grad.clone(), sets[0][1].grad.clone())
                path_b(sets[0])
                agree = all(torch.equal(x, y) for x, y in zip(ga, (sets[0][0].grad, sets[0][1].grad)))
                del ga
                for _, fn in variants:   # warm-up
                    time_ms(fn, sets, 1)
                t = {n: [] for n, _ in variants}
                for _ in range(args.rounds):
                    for n, fn in variants:
                        t[n].append(time_ms(fn, sets, 1))
                med = {n: sorted(v)[len(v) // 2] for n, v in t.items()}
                names = [n for n, _ in variants]
                say()
                say(f"-- {name} predictions, class_num = {class_num}, {kind}: (a) moves {moved / 1e6:.0f} MB; gradients of (a) and (b) "
                    f"torch.equal: {agree}")
                for n in names:
                    v = t[n]
                    extra = f"  {moved / (med[n] * 1e-3) / 1e9:6.0f} GB/s" if n.startswith(("(a)", "(e)")) else ""
                    say(f"  {n:46s} {med[n] * 1e3:9.1f} us  ({min(v) * 1e3:.1f} .. {max(v) * 1e3:.1f}){extra}")
                a, bb, c = names[0], names[1], names[2]
                spread = max(t[bb]) - min(t[bb])
                ok = med[bb] - med[a] > spread
                verdicts.append(ok and agree)
                say(f"  (b) / (a) = {med[bb] / med[a]:.2f};  (b) - (a) = {(med[bb] - med[a]) * 1e3:.1f} us against a spread of (b) of "
                    f"{spread * 1e3:.1f} us: (a) below (b) by more than that: {'yes' if ok else 'NO'};  (a) / (c) = {med[a] / med[c]:.3f};  "
                    f"(a) / (e) = {med[a] / med[names[5]]:.2f}")
                del sets, field, weights, tmp, half, half2
                torch.cuda.empty_cache()
    say()
    say(f"(a) below (b) by more than (b)'s spread, with equal gradients, in every case: {'yes' if all(verdicts) else 'NO'}")
    write_section(args.out, 1, lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "class_targets_probe.txt"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--b", type=int, default=32)
    ap.add_argument("--codegen", metavar="OTHER_TREE", help="compare head_targets.hip's assembly with that tree's instead of measuring")
    args = ap.parse_args()
    if args.codegen:
        codegen(os.path.abspath(args.codegen), args.out)
    else:
        measure(args)


if __name__ == "__main__":
    main()
