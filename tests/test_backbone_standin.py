"""The backbone half of the end-to-end timing (tools/e2e_amd.py) uses a stand-in written from the layer shapes, because the
reference's Python cannot travel to the GPU box.  HERE, where /root/reference exists, the stand-in is pinned against the reference's
own class: `Resnet18_8s` (lib/networks/model_repository.py:7-80, with `model_zoo.load_url` of lib/networks/resnet.py:231 stubbed --
there is no network) must have the same parameters and buffers in the same order, and with the stand-in's weights copied in, the
same outputs.  So what tools/e2e_amd.py times IS the reference's network (random weights), layer for layer.

Without the reference tree the same comparison runs against fixture G9 (tests/golden/backbone_resnet18_8s.npz, made by
tests/golden/make_golden.py from the reference's class): its parameter / buffer shapes in order, and its outputs on a seeded
input with the seeded stand-in's weights copied in."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"

SCRIPT = r"""
import sys, types, torch
sys.path.insert(0, %(tools)r); sys.path.insert(0, %(root)r)
import refshim
refshim.install(%(ref)r)
import e2e_amd                                   # the stand-in (imports the repo's own packages first)
for k in [k for k in sys.modules if k == "lib" or k.startswith("lib.")]:
    del sys.modules[k]                           # the repo's drop-in overlay package is also called `lib`
sys.path.insert(0, %(ref)r)
import lib.networks.resnet as R
R.model_zoo.load_url = lambda *a, **k: {}        # resnet.py:231 -- no network here
R.ResNet.load_state_dict = lambda self, sd, *a, **k: None
from lib.networks.model_repository import Resnet18_8s
torch.manual_seed(0)
ref = Resnet18_8s(ver_dim=18, seg_dim=2).eval()
mine = e2e_amd.StandInResnet18_8s(ver_dim=18, seg_dim=2).eval()
# the reference keeps ResNet's ImageNet head behind `fc` replaced (model_repository.py:23-27) and nothing else unused
rp = [(n, p) for n, p in ref.named_parameters()]
mp = [(n, p) for n, p in mine.named_parameters()]
rb = [(n, b) for n, b in ref.named_buffers()]
mb = [(n, b) for n, b in mine.named_buffers()]
assert [tuple(p.shape) for _, p in rp] == [tuple(p.shape) for _, p in mp], "parameter shapes / order differ"
assert [tuple(b.shape) for _, b in rb] == [tuple(b.shape) for _, b in mb], "buffer shapes / order differ"
with torch.no_grad():
    for m in mine.modules():   # non-trivial statistics and affine terms, so that every BatchNorm matters
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.normal_(0, 0.2); m.running_var.uniform_(0.5, 1.5); m.weight.uniform_(0.5, 1.5); m.bias.normal_(0, 0.2)
    for (_, a), (_, b) in zip(rp, mp):
        a.copy_(b)
    for (_, a), (_, b) in zip(rb, mb):
        a.copy_(b)
    x = torch.randn(2, 3, 64, 96)
    s0, v0 = ref(x)
    s1, v1 = mine(x)
print("params", sum(p.numel() for _, p in rp), "max |d seg|", float((s0 - s1).abs().max()), "max |d ver|", float((v0 - v1).abs().max()))
assert s0.shape == s1.shape == (2, 2, 64, 96) and v0.shape == v1.shape == (2, 18, 64, 96)
assert float(s0.abs().max()) > 1e-3 and float(v0.std()) > 1e-3
assert torch.allclose(s0, s1, atol=1e-5, rtol=1e-5) and torch.allclose(v0, v1, atol=1e-5, rtol=1e-5)
print("STANDIN_EQUALS_REFERENCE")
"""


FIXTURE = os.path.join(ROOT, "tests", "golden", "backbone_resnet18_8s.npz")


def seeded_standin():
    """the stand-in with seeded weights and non-trivial BatchNorm statistics, and the seeded input of fixture G9"""
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import e2e_amd
    torch.manual_seed(0)
    mine = e2e_amd.StandInResnet18_8s(ver_dim=18, seg_dim=2).eval()
    with torch.no_grad():
        for m in mine.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.normal_(0, 0.2); m.running_var.uniform_(0.5, 1.5); m.weight.uniform_(0.5, 1.5); m.bias.normal_(0, 0.2)
    return mine, torch.randn(1, 3, 32, 48)


def test_standin_backbone_is_the_references_resnet18_8s():
    import json
    import torch
    if os.path.isdir(REF):
        code = SCRIPT % dict(tools=os.path.join(ROOT, "tools"), root=ROOT, ref=REF)
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0 and "STANDIN_EQUALS_REFERENCE" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
    g = np.load(FIXTURE)
    mine, x = seeded_standin()
    assert [list(p.shape) for p in mine.parameters()] == json.loads(str(g["param_shapes"])), "parameter shapes / order differ"
    assert [list(b.shape) for b in mine.buffers()] == json.loads(str(g["buffer_shapes"])), "buffer shapes / order differ"
    np.testing.assert_array_equal(x.numpy(), g["x"])
    with torch.no_grad():
        s1, v1 = mine(x)
    s0, v0 = torch.from_numpy(g["seg"]), torch.from_numpy(g["ver"])
    assert s0.shape == s1.shape == (1, 2, 32, 48) and v0.shape == v1.shape == (1, 18, 32, 48)
    assert float(s0.abs().max()) > 1e-3 and float(v0.std()) > 1e-3
    assert torch.allclose(s0, s1, atol=1e-5, rtol=1e-5) and torch.allclose(v0, v1, atol=1e-5, rtol=1e-5)
