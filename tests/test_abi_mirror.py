"""CPU-only: the Python mirror of the C ABI (pvnet_amd/_abi.py) against include/pvnet_vote.h and include/pvnet_nn.h -- every mirrored
constant, the layout structure field by field, and a prototype for every declared function."""
import ctypes as C
import os
import re

from pvnet_amd import _abi, build, evaluation, pnp, voting

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "pvnet_vote.h")).read()
NN_HDR = open(os.path.join(ROOT, "include", "pvnet_nn.h")).read()


def test_every_mirrored_constant_equals_the_header():
    defines = re.findall(r"^#define\s+PVNET_((?:F|S|MASK|POSE_W|METRIC)_\w+|NUM_STAGES|VOTE_ABI_VERSION)\s+\(?(-?\d+)u?\)?", HDR, re.M)
    names = [n for n, _ in defines]
    assert len(names) == len(set(names))
    # the families are all there: 11 flags, 4 status bits, 6 mask codes, 3 weight kinds, 1 metric flag, the two scalars
    for family, count in (("F_", 11), ("S_", 4), ("MASK_", 6), ("POSE_W_", 3), ("METRIC_", 1)):
        assert sum(n.startswith(family) for n in names) == count, family
    assert "NUM_STAGES" in names and "VOTE_ABI_VERSION" in names
    for name, value in defines:
        mirror = "ABI_VERSION" if name == "VOTE_ABI_VERSION" else name
        assert getattr(_abi, mirror) == int(value), name
    assert _abi.F_CONCURRENT == 256 and _abi.ABI_VERSION == 9
    assert len(_abi.STAGE_NAMES) == _abi.NUM_STAGES
    # the error codes _check names
    errors = dict(re.findall(r"^#define\s+PVNET_(E_\w+)\s+\((-\d+)\)", HDR, re.M))
    assert set(errors) == {"E_BADARG", "E_WORKSPACE", "E_UNSUPPORTED"}
    for name, value in errors.items():
        assert getattr(_abi, name) == int(value) and _abi._ERROR_NAMES[int(value)] == "PVNET_" + name
    # the front end's modules hold the SAME objects, not copies typed again
    for mod, mirrored in ((voting, ("F_LITERAL", "F_CONCURRENT", "F_CULL_ALL", "S_SKIPPED", "S_OVERFLOW", "NUM_STAGES", "STAGE_NAMES",
                                    "Layout", "TUNING_KNOBS", "LIB_PATH", "DEV_LIB_PATH")),
                          (pnp, ("POSE_W_NONE", "POSE_W_EXPLICIT", "POSE_W_COV_F32")), (evaluation, ("METRIC_SYM_PROJECTION",))):
        for n in mirrored:
            assert getattr(mod, n) is getattr(_abi, n), (mod.__name__, n)
    assert voting._MASK_CODES[voting.torch.int64] == _abi.MASK_I64 and voting._MASK_CODES[voting.torch.float32] == _abi.MASK_F32


def test_layout_mirrors_the_header_structure_field_by_field():
    body = re.search(r"typedef struct PvnetVoteLayout \{(.*?)\} PvnetVoteLayout;", HDR, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for ctype, names in re.findall(r"\b(int32_t|size_t)\s+([\w\s,]+);", body):
        fields += [(n.strip(), {"int32_t": C.c_int32, "size_t": C.c_size_t}[ctype]) for n in names.split(",")]
    assert len(fields) == 33 and not re.sub(r"\b(int32_t|size_t)\s+[\w\s,]+;", "", body).strip()   # nothing of another type in it
    assert fields == list(_abi.Layout._fields_)


def test_every_declared_function_has_a_prototype():
    declared = set(re.findall(r"\b(pvnet_[a-z0-9_]+)\s*\(", HDR)) | set(re.findall(r"^(?:int|size_t)\s+(pvnet_[a-z0-9_]+)\s*\(", NN_HDR, re.M))
    assert {"pvnet_vote_v3", "pvnet_pose_solve", "pvnet_pose_metrics", "pvnet_vote_allgather", "pvnet_nearest_point_idx",
            "pvnet_nearest_workspace_bytes", "pvnet_motion_workspace_bytes"} <= declared
    assert declared == set(_abi.PROTOTYPES)
    returns = dict((n, t) for t, n in re.findall(r"^(int|size_t|void|const char\*)\s+(pvnet_[a-z0-9_]+)\s*\(", HDR + NN_HDR, re.M))
    assert set(returns) == declared
    want = {"int": C.c_int, "size_t": C.c_size_t, "void": None, "const char*": C.c_char_p}
    for name, (restype, argtypes) in _abi.PROTOTYPES.items():
        assert restype is want[returns[name]], name
        assert isinstance(argtypes, list)
    build.build()
    lib = voting.load_library()   # applied to the loaded library: a byte count is not cut to 32 bits
    for name, (restype, argtypes) in _abi.PROTOTYPES.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes or []) == argtypes, name
