"""Build-time check of every kernel's register accounting: the translation units of libpvnet_vote.so, release and development build,
and those of every side library (the rows of pvnet_amd.build.SIDE_LIBRARIES, one build each).

Rule: a kernel must not use the last VGPR granule of its allocation -- `.amdhsa_next_free_vgpr` has to exceed the highest
VGPR an instruction names by at least 8 (PVNET_SPARE_VGPRS in the sources provides the slack).  Background: round 2's
compaction flake (profiles/r02_compaction_flake_investigation.txt): identical code failed in 98 % of the runs with an
allocation that was used to the top and never with one granule more.

    python tools/check_kernel_resources.py            # compiles the sources of all of them to assembly (hipcc -S) and checks them
    python tools/check_kernel_resources.py --<name>   # one side library's translation units only (its build), e.g. --head
    python tools/check_kernel_resources.py a.s b.s

Second rule: the kernels whose budget is set with `amdgpu_num_vgpr` (hypothesis_kernel, score_exact_kernel_*) rely on
the gfx950 backend DOUBLING the attribute's literal (unified VGPR / AGPR file).  A compiler that stopped doing so would cap them at
half their registers: massive spilling.  So for those kernels the allocation must be EXACTLY the one the occupancy plan assumes
(EXPECTED_ALLOC: not more -- a wave per SIMD lost -- and not less), they must use more than half of it (a halved cap cannot) and
none of them may spill more than its own few dwords (`.amdhsa_private_segment_fixed_size`, limit per pattern in EXPECTED_ALLOC).

Third (tests/test_library_cpu.py, release_differs_from_dev): every kernel of the release build has the instruction stream and the
descriptor of the same-named development kernel -- the knob and fuzz tests, which load the development build, speak for the
shipped kernels only then.

Also reports the waves per SIMD each allocation permits (512 VGPRs per SIMD, granule 8).  Exit status 1 if a kernel lacks
the slack.  tests/test_library_cpu.py runs it on every build of the CPU suite.
"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLACK = 8
# kernels with an `amdgpu_num_vgpr` budget: name pattern -> the allocation (VGPRs, granule-rounded) their occupancy plan assumes, and
# the bytes per lane they may spill (per pattern -- the default dense kernels none to speak of: a spill in their loop is a
# regression; the two-pair variant five dwords; the hypothesis kernel ten, parked across its preamble (after the loads they hold have arrived); the merged dense + disc-culling kernel none: what the compiler used to hoist
# out of its two item loops and spill is made per use in the sources).  A halved cap spills hundreds.
EXPECTED_ALLOC = [(r"\d+hypothesis_kernelI", 48, 48), (r"score_exact_kernel_[12]_", 112, 12),
                  (r"score_exact_kernel_4_", 144, 12), (r"score_exact_kernel_8_\d_\d_1_0", 128, 12), (r"score_exact_kernel_8_\d_\d_1_1", 136, 12),
                  (r"score_exact_kernel_8_\d_\d_2_", 168, 24), (r"score_exact_kernel_both_\d_0", 128, 0), (r"score_exact_kernel_both_\d_1", 136, 0)]


def compile_to_asm(src, out, dev=False):
    sys.path.insert(0, ROOT)
    from pvnet_amd import build as B
    flags = [f for f in B.flags() if f not in ("-shared", "-fPIC")] + (["-DPVNET_DEV"] if dev else [])
    subprocess.check_call([B.hipcc_path()] + flags + ["-S", "--cuda-device-only", "-Wno-unused-command-line-argument", src, "-o", out],
                          stderr=subprocess.DEVNULL)


def kernels(text):
    """[(name, next_free_vgpr, highest VGPR named by an instruction)]"""
    out = []
    for m in re.finditer(r"\.amdhsa_kernel (\S+)", text):
        name = m.group(1)
        desc = text[m.start():text.index(".end_amdhsa_kernel", m.start())]
        nfv = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", desc).group(1))
        m2 = re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", desc)
        scratch = int(m2.group(1)) if m2 else 0
        i = text.index(name + ":")
        body = text[i:text.index(".Lfunc_end", i)]
        body = "\n".join(l.split(";")[0] for l in body.splitlines())  # comments may mention registers
        used = [int(x) for x in re.findall(r"\bv(\d+)\b", body)] + [int(b) for _, b in re.findall(r"\bv\[(\d+):(\d+)\]", body)]
        out.append((name, nfv, max(used) if used else -1, scratch))
    return out


def short(name):
    return re.sub(r"^_ZN(3pvd)?\d+_GLOBAL__N_1\d+", "", name)[:56]


_ASM = None   # [(translation unit, dev, assembly)] of this process: compiled once, shared by main() and the CPU tests


def assembly():
    """[(translation unit, dev, assembly text)]: the release and development (-DPVNET_DEV) instantiations of every translation unit
    of libpvnet_vote.so, compiled to assembly with the product's flags (once per process)"""
    global _ASM
    if _ASM is None:
        sys.path.insert(0, ROOT)
        from pvnet_amd import build as B
        with tempfile.TemporaryDirectory() as d:
            from concurrent.futures import ThreadPoolExecutor
            jobs = [(src, dev, os.path.join(d, f"k{k}{'d' if dev else ''}.s")) for k, src in enumerate(B.SRC) for dev in (False, True)
                    if "rccl" not in src]
            with ThreadPoolExecutor(max_workers=max(1, min(16, (os.cpu_count() or 4) - 1))) as ex:
                list(ex.map(lambda j: compile_to_asm(j[0], j[2], j[1]), jobs))
            _ASM = [(src, dev, open(out).read()) for src, dev, out in jobs]
    return _ASM


def side_assembly(name):
    """[(translation unit, assembly text)] of one of build.SIDE_LIBRARIES (one build each, no development variant)"""
    sys.path.insert(0, ROOT)
    from pvnet_amd import build as B
    out = []
    with tempfile.TemporaryDirectory() as d:
        for k, src in enumerate(B._side(name)[0]):
            compile_to_asm(src, os.path.join(d, f"{name}{k}.s"))
            out.append((src, open(os.path.join(d, f"{name}{k}.s")).read()))
    return out


def kernel_code(text):
    """{kernel: (instruction stream, .amdhsa_* descriptor fields)} of one assembly file -- comments and directives stripped, local
    labels (.LBB3_7, .Ltmp12, ...) renamed in order of appearance, so two compilations of one kernel compare equal however the rest of
    their translation units numbered their labels"""
    out = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)", text):
        name = m.group(1)
        desc = text[m.start():text.index(".end_amdhsa_kernel", m.start())]
        fields = tuple(l.strip() for l in desc.splitlines() if l.strip().startswith(".amdhsa_"))
        i = text.index("\n" + name + ":") + 1
        labels = {}
        code = []
        for line in text[i:text.index(".Lfunc_end", i)].splitlines():
            line = line.split(";")[0].strip()
            if not line or (line.startswith(".") and not re.match(r"\.L\w+:$", line)):
                continue
            code.append(re.sub(r"\.L\w+", lambda lm: labels.setdefault(lm.group(0), f".L{len(labels)}"), line))
        out[name] = (tuple(code), fields)
    return out


def release_differs_from_dev(pairs):
    """pairs: [(release assembly, development assembly)] of the same translation units -> the kernels of the release build whose
    instruction stream or descriptor differs from the same-named kernel of the development build (or that it lacks).  The knob and
    fuzz tests run the development build: what they show holds for the shipped kernels only while this list is empty."""
    bad = []
    for rel, dev in pairs:
        kd = kernel_code(dev)
        for name, code in kernel_code(rel).items():
            if kd.get(name) != code:
                bad.append(name)
    return bad


def main(argv):
    sys.path.insert(0, ROOT)
    from pvnet_amd import build as B
    if len(argv) == 1 and argv[0].startswith("--") and argv[0][2:] in B.SIDE_LIBRARIES:
        texts = [t for _, t in side_assembly(argv[0][2:])]
    elif argv:
        texts = [open(a).read() for a in argv]
    else:
        texts = [t for _, _, t in assembly()] + [t for name in B.SIDE_LIBRARIES for _, t in side_assembly(name)]
    bad = 0
    n = 0
    done = set()
    for t in texts:
        for name, nfv, vmax, scratch in kernels(t):
            if (name, nfv, vmax, scratch) in done:   # the same kernel in the release and the development build
                continue
            done.add((name, nfv, vmax, scratch))
            n += 1
            slack = nfv - (vmax + 1)
            alloc = (nfv + 7) // 8 * 8
            flag = "" if slack >= SLACK else "   <-- uses its last granule: raise PVNET_SPARE_VGPRS"
            bad += slack < SLACK
            for pat, want, max_scratch in EXPECTED_ALLOC:
                if re.search(pat, name):
                    if alloc != want or vmax + 1 <= want // 2 or scratch > max_scratch:
                        flag += f"   <-- budgeted kernel: expected {want} VGPRs allocated, more than {want // 2} used, no scratch (got {alloc}, {vmax + 1}, {scratch} B)"
                        bad += 1
                    break
            print(f"{short(name):58s} uses v0..v{vmax:<3d} allocates {alloc:3d} (slack {slack:3d}, {min(8, 512 // alloc)} waves/SIMD, scratch {scratch:3d} B){flag}")
    print(f"checked {n} kernels, {bad} without a spare granule / off their register budget")
    return 1 if bad or n == 0 else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
