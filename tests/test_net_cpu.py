"""CPU-only checks of the fused network class (pvnet_amd/net.py): ``FusedNet`` and its four presets ``FusedTailNet``, ``FusedDecoderNet``,
``FusedStemNet``, ``FusedTrunkNet`` -- where the names live and how they relate, their arguments and refusals, the parameters they keep,
that with float32 features on the CPU every preset calls the stand-in's own modules in the stand-in's own order, and both attribute
spellings of the wrapped network (the reference's own class where its tree is present).  The parameter classes are tested in
tests/test_{tail,decoder,stem,trunk}_cpu.py."""
import os
import re
import subprocess
import sys

import pytest

torch = pytest.importorskip("torch")
from torch import nn  # noqa: E402

import pvnet_amd  # noqa: E402
from pvnet_amd import decoder as D, net as N, stem as S, tail as TL, trunk as T  # noqa: E402
from tests import tail_cases as TC  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
PRESETS = {"FusedTailNet": TL, "FusedDecoderNet": D, "FusedStemNet": S, "FusedTrunkNet": T}   # the name and the module it is read from
names = pytest.mark.parametrize("name", list(PRESETS))


@pytest.fixture(scope="module")
def standin():
    return TC.standin()   # the seeded stand-in and its 1 x 3 x 32 x 48 input


def test_the_names_their_modules_and_their_relations():
    for name, module in PRESETS.items():
        cls = getattr(N, name)
        assert getattr(module, name) is cls and getattr(pvnet_amd, name) is cls and issubclass(cls, N.FusedNet) and name in pvnet_amd.__all__
    assert pvnet_amd.FusedNet is N.FusedNet and "FusedNet" in pvnet_amd.__all__
    assert issubclass(N.FusedStemNet, N.FusedDecoderNet) and issubclass(N.FusedTrunkNet, N.FusedStemNet)
    assert not issubclass(N.FusedDecoderNet, N.FusedTailNet)
    with pytest.raises(AttributeError):
        TL.FusedDecoderNet
    # no cycle at module load, whichever module comes first; and the four do not import each other
    for order in ("trunk, pvnet_amd.tail", "tail, pvnet_amd.trunk", "stem", "net"):
        code = f"import pvnet_amd.{order}; from pvnet_amd.stem import FusedStemNet; from pvnet_amd.decoder import FusedDecoderNet"
        subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT, timeout=300)
    for module in PRESETS.values():
        text = open(module.__file__).read()
        assert not any(f"from .{other}" in text for other in ("tail", "decoder", "stem", "trunk"))
    for module in (N, *PRESETS.values()):   # no method is assigned in __init__
        assert not re.search(r"self\._(stem|trunk|features|layer)\s*=", open(module.__file__).read())


def test_the_parameters_each_preset_keeps(standin):
    net, _ = standin
    tail = N.FusedTailNet(net)
    assert tail.seg_dim == 2 and tail.params is tail.tail_params and (tail.stem, tail.layers, tail.stages) == (False, (), ())
    dec = N.FusedDecoderNet(net)
    assert dec.seg_dim == 2 and dec.stages == D.DEFAULT_STAGES and set(dec.stages) <= set(D.STAGES) and set(dec.stage_params) == set(dec.stages)
    assert N.FusedDecoderNet(net, stages=()).stage_params == {} and (dec.stem, dec.layers) == (False, ())
    stem = N.FusedStemNet(net)
    assert isinstance(stem, N.FusedDecoderNet) and stem.stem is S.DEFAULT_STEM and stem.stages == D.DEFAULT_STAGES and stem.layers == ()
    assert (stem.stem_params is not None) == S.DEFAULT_STEM and N.FusedStemNet(net, stem=False).stem_params is None
    every = N.FusedTrunkNet(net, layers=T.LAYERS)
    assert set(every.blocks) == set(T.LAYERS[:4]) and all(len(v) == 2 for v in every.blocks.values())
    assert (every.fc_params.cin, every.fc_params.co, every.fc_params.act) == (512, 256, "relu")
    assert (every.conv8s_params.cin, every.conv8s_params.co, every.conv8s_params.act) == (384, 128, "leaky")
    none = N.FusedTrunkNet(net, layers=())
    assert len(none.blocks) == 0 and none.fc_params is None and none.conv8s_params is None
    assert set(T.DEFAULT_LAYERS) <= set(T.LAYERS) and N.FusedTrunkNet(net).layers == T.DEFAULT_LAYERS
    full = N.FusedNet(net)
    assert (full.stem, full.layers, full.stages, full.precision) == (S.DEFAULT_STEM, T.DEFAULT_LAYERS, D.DEFAULT_STAGES, None)
    for fused in (tail, dec, stem, every, none, full):
        assert fused.net is net and isinstance(fused.parts, N.NetworkParts) and isinstance(fused.tail_params, TL.TailParams)


class Decoder(nn.Module):
    """the decoder's attributes without a trunk of either spelling"""

    def __init__(self, net):
        super().__init__()
        self.seg_dim, self.conv4s, self.conv2s, self.convraw = net.seg_dim, net.conv4s, net.conv2s, net.convraw


class ReferenceSpelled(nn.Module):
    """the reference's attribute names over the stand-in's modules, its two switches included"""

    def __init__(self, net, **switches):
        super().__init__()
        t = self.resnet18_8s = nn.Module()
        (t.conv1, t.bn1, t.relu), t.maxpool, t.fc = net.stem, net.pool, net.fc
        t.layer1, t.layer2, t.layer3, t.layer4 = net.l1, net.l2, net.l3, net.l4
        t.fully_conv, t.remove_avg_pool_layer = switches.get("fully_conv", True), switches.get("remove_avg_pool_layer", True)
        self.up8sto4s = self.up4sto2s = self.up2storaw = net.up
        self.seg_dim, self.conv8s, self.conv4s, self.conv2s, self.convraw = net.seg_dim, net.conv8s, net.conv4s, net.conv2s, net.convraw


@names
def test_refusals(standin, name):
    net, x = standin
    cls = getattr(PRESETS[name], name)
    with pytest.raises(ValueError, match="precision"):
        cls(net, precision="fp8")
    if name != "FusedTailNet":
        with pytest.raises(ValueError, match="stages"):
            cls(net, stages=("conv8s",))
        with pytest.raises(ValueError, match="stages"):
            cls(net, stages=("conv2s", "conv2s"))
    if name == "FusedTrunkNet":
        with pytest.raises(ValueError, match="layers"):
            cls(net, layers=("layer5",))
    with pytest.raises(ValueError, match=f"{name}: neither"):
        cls(Decoder(net).eval())
    # a reference trunk that is not the fully convolutional one: every preset runs the trunk piece by piece, so every one refuses it
    for switch in ("fully_conv", "remove_avg_pool_layer"):
        with pytest.raises(ValueError, match=f"{name}: .*fully_conv=True, remove_avg_pool_layer=True"):
            cls(ReferenceSpelled(net, **{switch: False}).eval())
    fused = cls(net)
    net.train()
    try:
        with pytest.raises(RuntimeError, match=f"{name} is inference only"):
            fused(x)
    finally:
        net.eval()


def calls(net, run):
    """the ordered (leaf module, its inputs' shapes) that ``run()`` calls"""
    seen, hooks = [], []
    for m in net.modules():
        if not list(m.children()):
            hooks.append(m.register_forward_hook(lambda mod, args, out: seen.append((mod, tuple(tuple(a.shape) for a in args)))))
    try:
        with torch.no_grad():
            run()
    finally:
        for h in hooks:
            h.remove()
    return seen


def test_with_float32_features_every_preset_is_the_standins_own_modules_in_its_own_order(standin):
    """Float32 features on the CPU, no precision forced: the tier serves nothing, so whatever is named, ``_features`` is the wrapped
    modules.  The same leaf modules on the same shapes in the same order as the stand-in's own forward up to ``conv2s`` -- "with
    nothing named it is the same network" said of what runs, and the features are then the stand-in's bit for bit."""
    net, x = standin
    own = calls(net, lambda: net(x))
    last = max(k for k, (m, _) in enumerate(own) if m is net.conv2s[-1])
    own = own[:last + 1]
    # the stem's 3 and the pool, 8 blocks of 4 with 3 downsamples of 2, fc, conv8s, conv4s and conv2s of 3 each, 2 upsamples
    assert len(own) == 4 + 8 * 4 + 3 * 2 + 4 * 3 + 2 and own[0] == (net.stem[0], ((1, 3, 32, 48),)) and sum(m is net.up for m, _ in own) == 2
    want = TC.standin_features(net, x)
    for what, fused in {"FusedTrunkNet, none": N.FusedTrunkNet(net, layers=()), "FusedTrunkNet, all": N.FusedTrunkNet(net, layers=T.LAYERS),
                        "FusedTrunkNet, no stem": N.FusedTrunkNet(net, layers=T.LAYERS, stem=False), "FusedStemNet": N.FusedStemNet(net),
                        "FusedStemNet, stem": N.FusedStemNet(net, stem=True), "FusedDecoderNet": N.FusedDecoderNet(net),
                        "FusedTailNet": N.FusedTailNet(net), "FusedNet": N.FusedNet(net)}.items():
        assert calls(net, lambda: fused._features(x)) == own, what
        with torch.no_grad():
            assert fused._stem_dtype(x) is None and torch.equal(fused._features(x), want), what
            trunk = fused._trunk(x)
            assert [tuple(t.shape) for t in trunk] == [(1, 128, 4, 6), (1, 64, 8, 12), (1, 64, 16, 24)]
            for a, b_ in zip(trunk, N.FusedDecoderNet(net)._trunk(x)):   # the float32 trunk is the decoder net's
                assert torch.equal(a, b_), what


REFERENCE_SCRIPT = r"""
import sys, torch
sys.path.insert(0, %(tools)r); sys.path.insert(0, %(root)r)
import refshim
refshim.install(%(ref)r)
from tests import tail_cases as TC
from pvnet_amd import decoder as D, net as N, stem as S, tail as TL, trunk as T
mine, x = TC.standin()
for k in [k for k in sys.modules if k == "lib" or k.startswith("lib.")]:
    del sys.modules[k]                           # the repo's drop-in overlay package is also called `lib`
sys.path.insert(0, %(ref)r)
import lib.networks.resnet as R
R.model_zoo.load_url = lambda *a, **k: {}        # no network here
R.ResNet.load_state_dict = lambda self, sd, *a, **k: None
from lib.networks.model_repository import Resnet18_8s
ref = Resnet18_8s(ver_dim=18, seg_dim=2).eval()
with torch.no_grad():
    for a, b in zip(ref.parameters(), mine.parameters()):
        a.copy_(b)
    for a, b in zip(ref.buffers(), mine.buffers()):
        a.copy_(b)
same = lambda p, q, names: all(torch.equal(getattr(p, n), getattr(q, n)) for n in names)
assert same(TL.TailParams.from_network(ref), TL.TailParams.from_network(mine), ("w1", "b1", "w2", "b2"))
assert same(S.StemParams.from_network(ref), S.StemParams.from_network(mine), ("w", "bias"))
for stage in D.STAGES:
    assert same(D.StageParams.from_network(ref, stage), D.StageParams.from_network(mine, stage), ("w", "bias", "packed"))
Fr, Fm = N.FusedTrunkNet(ref, layers=T.LAYERS), N.FusedTrunkNet(mine, layers=T.LAYERS)
for name in T.LAYERS[:4]:
    for br, bm, blk in zip(Fr.blocks[name], Fm.blocks[name], getattr(ref.resnet18_8s, name)):
        assert isinstance(blk, R.BasicBlock)     # the reference's own class
        assert same(br.conv1, bm.conv1, ("packed", "bias")) and same(br.conv2, bm.conv2, ("packed", "bias"))
        assert (br.down is None) == (bm.down is None) and (br.down is None or torch.equal(br.down[0], bm.down[0]))
assert torch.equal(Fr.fc_params.packed, Fm.fc_params.packed) and torch.equal(Fr.conv8s_params.packed, Fm.conv8s_params.packed)
try:
    T.FusedBasicBlock(R.Bottleneck(64, 16))
    raise SystemExit("the Bottleneck was taken")
except ValueError:
    pass
with torch.no_grad():
    whole = ref.resnet18_8s(x)                   # the one call the reference's network makes: x2s, x4s, x8s, x16s, x32s, xfc
    whole = (ref.conv8s(torch.cat([whole[5], whole[2]], 1)), whole[1], whole[0])
    for make in (N.FusedTailNet, N.FusedDecoderNet, N.FusedStemNet, N.FusedTrunkNet, N.FusedNet):
        tr, tm = make(ref)._trunk(x), make(mine)._trunk(x)   # conv8s' output and the two skips, under the reference's attribute names
        assert [tuple(t.shape) for t in tr] == [(1, 128, 4, 6), (1, 64, 8, 12), (1, 64, 16, 24)]
        assert all(torch.allclose(a, b, atol=1e-5, rtol=1e-5) for a, b in zip(tr, tm))
        assert all(torch.equal(a, b) for a, b in zip(tr, whole))   # piecewise, the reference's own forward
        fr, fm = make(ref)._features(x), make(mine)._features(x)   # float32 features: the reference's own up8sto4s / conv4s / up4sto2s / conv2s
        assert fr.shape == (1, 32, 16, 24) and torch.allclose(fr, fm, atol=1e-5, rtol=1e-5)
# a trunk that is not the fully convolutional one is refused, under every name
for make in (N.FusedTailNet, N.FusedDecoderNet, N.FusedStemNet, lambda net: N.FusedStemNet(net, stem=False), N.FusedTrunkNet, N.FusedNet):
    for switches in ((True, False), (False, True)):
        plain = Resnet18_8s(ver_dim=18, seg_dim=2).eval()
        plain.resnet18_8s.fully_conv, plain.resnet18_8s.remove_avg_pool_layer = switches
        try:
            make(plain)
        except ValueError as e:
            assert "fully_conv" in str(e)
        else:
            raise AssertionError("not refused")
print("BOTH_SPELLINGS")
"""


def test_every_preset_takes_the_references_spelling_and_its_own_class_where_its_tree_is_present(standin):
    net, x = standin
    spelled, want = ReferenceSpelled(net).eval(), TC.standin_features(net, x)
    with torch.no_grad():   # the reference's names over the same modules: the same bits
        assert all(torch.equal(getattr(N, name)(spelled)._features(x), want) for name in PRESETS)
    if not os.path.isdir(REF):
        return
    code = REFERENCE_SCRIPT % dict(tools=os.path.join(ROOT, "tools"), root=ROOT, ref=REF)   # loaded the way tests/test_backbone_standin.py loads it
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0 and "BOTH_SPELLINGS" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
