"""CPU-only checks that hold for EVERY side library (the rows of pvnet_amd.build.SIDE_LIBRARIES and pvnet_amd._abi.SIDE_LIBRARIES),
parametrised over the registry: its header against its prototype table, its table against every other table, the built library, the
register check for it alone and within the no-argument run, and the loud failure without it.  What is particular to one library --
parameter positions, constants, structs, kernel names and counts, bad arguments -- is in that library's own test file."""
import contextlib
import ctypes as C
import importlib.util
import io
import os
import re
import subprocess
import sys

import pytest

from pvnet_amd import _abi, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "check_kernel_resources.py")
NAMES = sorted(build.SIDE_LIBRARIES)
side = pytest.mark.parametrize("name", NAMES)


def test_the_two_halves_of_the_registry_have_the_same_keys():
    assert list(build.SIDE_LIBRARIES) == list(_abi.SIDE_LIBRARIES) and len(NAMES) >= 7
    for name, (path, version, table) in _abi.SIDE_LIBRARIES.items():
        assert path == build._side(name)[2] and path.endswith(f"libpvnet_{name}.so")
        # the names front ends and tests import are the registry's values, and the public loader is the registry's
        assert getattr(_abi, f"{name.upper()}_LIB_PATH") == path and getattr(_abi, f"{name.upper()}_ABI_VERSION") == version
        assert getattr(_abi, f"{name.upper()}_PROTOTYPES") is table
        assert callable(getattr(_abi, f"load_{name}_library"))


def test_the_shared_warp_header_rebuilds_exactly_the_two_libraries_that_compile_it():
    shared = os.path.join(build.CSRC, "augment_warp.h")
    assert os.path.exists(shared)
    assert {n for n in build.SIDE_LIBRARIES if shared in build._side(n)[1]} == {"augment", "color"}
    for name in NAMES:   # every library depends on its sources and its own header, and every dependency exists
        src, deps, _ = build._side(name)
        assert set(src) <= set(deps) and os.path.join(ROOT, "include", build.SIDE_LIBRARIES[name][1]) in deps
        assert all(os.path.exists(d) for d in deps), name
        assert not {os.path.basename(s) for s in src} & set(build.VOTE_TU)


@side
def test_header_declares_the_exports_and_every_one_has_a_prototype(name):
    hdr = open(os.path.join(ROOT, "include", build.SIDE_LIBRARIES[name][1])).read()
    _, version, table = _abi.SIDE_LIBRARIES[name]
    returns = dict((n, t) for t, n in re.findall(r"^(int|size_t)\s+(pvnet_[a-z0-9_]+)\s*\(", hdr, re.M))
    assert set(returns) == set(table) and f"pvnet_{name}_abi_version" in table
    want = {"int": C.c_int, "size_t": C.c_size_t}
    for fn, (restype, argtypes) in table.items():
        assert restype is want[returns[fn]], fn
        decl = re.search(r"^(?:int|size_t)\s+%s\s*\((.*?)\);" % fn, hdr, re.M | re.S).group(1)
        assert len(argtypes) == (0 if decl.strip() == "void" else len(decl.split(","))), fn   # one argument type per parameter
    assert int(re.search(r"^#define\s+PVNET_%s_ABI_VERSION\s+(\d+)" % name.upper(), hdr, re.M).group(1)) == version


@side
def test_table_shares_no_name_with_any_other(name):
    others = set(_abi.PROTOTYPES).union(*(t.prototypes for n, t in _abi.SIDE_LIBRARIES.items() if n != name))
    assert not set(_abi.SIDE_LIBRARIES[name].prototypes) & others


@pytest.fixture(scope="module")
def built():
    build.build()


@side
def test_library_is_built_for_gfx950_and_exports_the_symbols_bound_once(name, built):
    path, version, table = _abi.SIDE_LIBRARIES[name]
    assert os.path.exists(path) and b"gfx950" in open(path, "rb").read()
    raw, lib = C.CDLL(path), getattr(_abi, f"load_{name}_library")()
    assert lib is _abi._load_side(name)   # loaded once
    for fn, (restype, argtypes) in table.items():
        assert hasattr(raw, fn), fn
        bound = getattr(lib, fn)          # bound once, at load
        assert bound.restype is restype and list(bound.argtypes or []) == argtypes, fn
    assert getattr(lib, f"pvnet_{name}_abi_version")() == version
    # no other library of the project exports any of its names
    for other in [_abi.LIB_PATH, _abi.DEV_LIB_PATH] + [t.path for n, t in _abi.SIDE_LIBRARIES.items() if n != name]:
        assert not any(hasattr(C.CDLL(other), fn) for fn in table), other


@side
def test_missing_library_fails_loudly(name, monkeypatch, tmp_path):
    monkeypatch.delitem(_abi._side_libs, name, raising=False)
    monkeypatch.setitem(_abi.SIDE_LIBRARIES, name, _abi.SIDE_LIBRARIES[name]._replace(path=str(tmp_path / "nope.so")))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        getattr(_abi, f"load_{name}_library")()


# ---- the register check ---------------------------------------------------------------------------------------------------------------
def printed(stdout):
    """the kernels a run of the tool printed (one line each, the name first), and the count its last line states"""
    names = [line.split()[0] for line in stdout.splitlines() if " allocates " in line]
    assert int(re.search(r"checked (\d+) kernels, 0 without", stdout).group(1)) == len(names)
    return set(names)


@pytest.fixture(scope="module")
def register_runs(built):
    """the tool's own output: ``--<name>`` for every library (a process each, as the build runs it), and the no-argument run"""
    spec = importlib.util.spec_from_file_location("check_kernel_resources", TOOL)
    chk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(chk)
    runs = {name: subprocess.run([sys.executable, TOOL, "--" + name], capture_output=True, text=True) for name in NAMES}
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        status = chk.main([])
    return chk, runs, status, buf.getvalue()


@side
def test_register_check_selects_that_library_alone_and_passes(name, register_runs):
    chk, runs, _, _ = register_runs
    r = runs[name]
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    asm, own = chk.side_assembly(name), set()
    assert [os.path.basename(src) for src, _ in asm] == build.SIDE_LIBRARIES[name][0]
    for _, text in asm:
        for kernel, nfv, vmax, scratch in chk.kernels(text):
            assert nfv - (vmax + 1) >= chk.SLACK, kernel
            own.add(chk.short(kernel))
    assert own and printed(r.stdout) == own   # every kernel printed comes from its translation units, and every one of them is printed
    for other in NAMES:
        if other != name:
            assert not printed(runs[other].stdout) & own, other


def test_no_argument_run_is_the_vote_library_and_every_side_library(register_runs):
    chk, runs, status, stdout = register_runs
    assert status == 0
    vote = {chk.short(k[0]) for _, _, text in chk.assembly() for k in chk.kernels(text)}
    assert vote and printed(stdout) == vote.union(*(printed(r.stdout) for r in runs.values()))
    assert not any(vote & printed(r.stdout) for r in runs.values())
