"""CPU-only checks of what the four fused network wrappers share (pvnet_amd/_net.py): the BatchNorm fold against torch's own eval()
BatchNorm in float64, the four parameter classes' tensors against the digests recorded before the plumbing was shared
(tests/golden/net_params_parent.json, written by tests/golden/make_net_params_golden.py), and ``NetworkParts``' resolution of both
spellings of the wrapped network (the reference's own class where its tree is present)."""
import importlib.util
import json
import os
import subprocess
import sys

import pytest

torch = pytest.importorskip("torch")
import torch.nn.functional as F  # noqa: E402
from torch import nn  # noqa: E402

from pvnet_amd import _net  # noqa: E402
from tests import tail_cases, trunk_cases  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
GOLDEN = os.path.join(ROOT, "tests", "golden", "net_params_parent.json")

# (cin, cout, kernel, stride, padding, the input's sides): a trunk 3 x 3, the stem's 7 x 7 stride 2, a block's 1 x 1 downsample
CONVS = {"3x3": (64, 96, 3, 1, 1, (9, 11)), "7x7/2": (3, 64, 7, 2, 3, (21, 27)), "1x1 downsample": (64, 128, 1, 2, 0, (9, 12))}


@pytest.mark.parametrize("affine", [True, False], ids=["affine", "no affine"])
@pytest.mark.parametrize("kind", list(CONVS))
def test_fold_against_torchs_own_eval_batchnorm_in_float64(kind, affine):
    cin, cout, k, s, p, (h, w) = CONVS[kind]
    torch.manual_seed(11)
    conv, bn = nn.Conv2d(cin, cout, k, s, p, bias=False), nn.BatchNorm2d(cout, affine=affine).eval()
    with torch.no_grad():
        bn.running_mean.normal_(0, 0.3); bn.running_var.uniform_(0.3, 2.0)
        if affine:
            bn.weight.uniform_(0.5, 1.5); bn.bias.normal_(0, 0.3)
    _net.check_conv_bn("test", conv, bn)
    wf, bf = _net.fold_batchnorm(conv, bn)
    assert wf.dtype == bf.dtype == torch.float32 and wf.shape == conv.weight.shape and tuple(bf.shape) == (cout,)
    x = torch.randn(2, cin, h, w, dtype=torch.float64)
    with torch.no_grad():
        want = bn.double()(conv.double()(x))
        got = F.conv2d(x, wf.double(), bf.double(), stride=s, padding=p)
        # the folded values are float64 values rounded once to float32: 2^-24 of every term
        lim = 2.0 ** -24 * F.conv2d(x.abs(), wf.double().abs(), bf.double().abs(), stride=s, padding=p) + 1e-14
        assert ((got - want).abs() <= lim).all()
        assert float((got - want).abs().max()) > 0   # (it IS rounded: not the float64 fold itself)
        # and they are the one rounding of the float64 fold, value by value
        sc = (bn.weight if affine else torch.ones(cout, dtype=torch.float64)) / torch.sqrt(bn.running_var + bn.eps)
        assert torch.equal(wf, (conv.weight * sc[:, None, None, None]).float())
        assert torch.equal(bf, ((bn.bias if affine else 0.0) - bn.running_mean * sc).float())


def test_the_four_parameter_classes_give_the_recorded_bits():
    spec = importlib.util.spec_from_file_location("make_net_params_golden", os.path.join(ROOT, "tests", "golden", "make_net_params_golden.py"))
    maker = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(maker)
    with open(GOLDEN) as fh:
        want = json.load(fh)
    got = maker.digests()
    assert set(got) == set(want) and len(want) == 72
    assert {k for k in want if got[k] != want[k]} == set()


def test_network_parts_resolves_the_standin_and_refuses_neither_spelling():
    for net in (tail_cases.standin()[0], trunk_cases.standin()):
        P = _net.NetworkParts(net)
        assert P.whole is None and all(a is b for a, b in zip(P.stem_triple, net.stem)) and len(P.stem_triple) == 3
        assert P.pool is net.pool and P.fc is net.fc and P.conv8s is net.conv8s and P.convraw is net.convraw
        assert all(a is b for a, b in zip(P.layers, (net.l1, net.l2, net.l3, net.l4))) and len(P.layers) == 4
        assert all(u is net.up for u in P.ups) and len(P.ups) == 3 and P.stages[0] is net.conv4s and P.stages[1] is net.conv2s
        blk = net.l2[0]
        assert all(a is b for a, b in zip(P.basic_block(blk), (blk.c1, blk.b1, blk.c2, blk.b2, blk.down)))
        P.require_fully_conv("test")   # the stand-in has no such switch
        x = tail_cases.standin()[1]
        with torch.no_grad():   # the wrapped modules in the stand-in's own order: the same bits
            x2s, p = P.eager_stem(x)
            x4s = P.layers[0](p)
            x8s = P.layers[1](x4s)
            xfc = P.fc(P.layers[3](P.layers[2](x8s)))
            fm = P.eager_stage(1, P.eager_stage(0, P.eager_conv8s(xfc, x8s), x4s), x2s)
            assert torch.equal(fm, tail_cases.standin_features(net, x))

    class Decoder(nn.Module):   # the decoder's attributes without a trunk of either spelling
        def __init__(self):
            super().__init__()
            self.seg_dim, self.conv4s, self.conv2s, self.convraw = net.seg_dim, net.conv4s, net.conv2s, net.convraw

    for neither in (nn.Sequential(), Decoder(), object()):
        with pytest.raises(ValueError, match="neither"):
            _net.NetworkParts(neither)
    with pytest.raises(ValueError, match="neither"):
        _net.NetworkParts.basic_block(nn.Sequential())


REFERENCE_SCRIPT = r"""
import sys, torch
sys.path.insert(0, %(tools)r); sys.path.insert(0, %(root)r)
import refshim
refshim.install(%(ref)r)
from pvnet_amd import _net
for k in [k for k in sys.modules if k == "lib" or k.startswith("lib.")]:
    del sys.modules[k]                           # the repo's drop-in overlay package is also called `lib`
sys.path.insert(0, %(ref)r)
import lib.networks.resnet as R
R.model_zoo.load_url = lambda *a, **k: {}        # no network here
R.ResNet.load_state_dict = lambda self, sd, *a, **k: None
from lib.networks.model_repository import Resnet18_8s
ref = Resnet18_8s(ver_dim=18, seg_dim=2).eval()
t, P = ref.resnet18_8s, _net.NetworkParts(ref)
assert P.whole is t and P.stem_triple == (t.conv1, t.bn1, t.relu) and P.pool is t.maxpool and P.fc is t.fc
assert P.layers == (t.layer1, t.layer2, t.layer3, t.layer4) and P.ups == (ref.up8sto4s, ref.up4sto2s, ref.up2storaw)
assert P.conv8s is ref.conv8s and P.stages == (ref.conv4s, ref.conv2s) and P.convraw is ref.convraw
blk = t.layer2[0]
assert isinstance(blk, R.BasicBlock) and P.basic_block(blk) == (blk.conv1, blk.bn1, blk.conv2, blk.bn2, blk.downsample)
P.require_fully_conv("test")
t.fully_conv = False
try:
    P.require_fully_conv("test")
except ValueError as e:
    assert "fully_conv" in str(e)
else:
    raise AssertionError("not refused")
print("REFERENCE_SPELLING")
"""


def test_network_parts_resolves_the_references_own_class_where_its_tree_is_present():
    if not os.path.isdir(REF):
        pytest.skip("the reference tree is not present")
    code = REFERENCE_SCRIPT % dict(tools=os.path.join(ROOT, "tools"), root=ROOT, ref=REF)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0 and "REFERENCE_SPELLING" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
