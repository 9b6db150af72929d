"""GPU tests of the fused network class (pvnet_amd/net.py) under its four preset names, against the eager stand-in.

No tolerance here is measured on the device code.  Under ``autocast(bfloat16)`` the bar is 2 e, where e is what the EAGER network under
the same autocast differs from the eager float32 network by: two differently ordered bfloat16 computations of the same function may each
sit e from it.  With float32 features the wrapped modules and the float32 tail run, under fixture G9's 1e-5.  A preset with nothing more
named than the preset below it is that preset, bit for bit.  The launches themselves are held to their restatements in
tests/test_{tail,decoder,stem,trunk}_device.py."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import tail_cases as TC  # noqa: E402
from tests import tail_restatement as TR  # noqa: E402


def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def case():
    """(pvnet_amd.net, the stand-in and its 1 x 3 x 32 x 48 input on the device, the eager float32 outputs in float64, e)"""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from pvnet_amd import net as N
    net, x = TC.standin()
    assert tuple(x.shape) == (1, 3, 32, 48)
    net, x = net.to(dev()), x.to(dev())
    with torch.no_grad():
        ref = torch.cat(net(x), 1).double()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            eager = torch.cat(net(x), 1)
    # e: what the EAGER network under the same autocast differs from the eager float32 network by
    e = float((eager.double() - ref).abs().max())
    assert e > 0
    return N, net, x, ref, e


def autocast(fused, x):
    with torch.autocast("cuda", dtype=torch.bfloat16):
        return fused(x)


def worst(y, ref):
    return float((torch.cat(tuple(y), 1).double() - ref).abs().max())


def hold(case, fused, what):
    """what every preset owes: under autocast bfloat16 views of one tensor within 2 e, with float32 features float32 within 1e-5"""
    _, _, x, ref, e = case
    seg, ver = autocast(fused, x)
    torch.cuda.synchronize()
    assert tuple(seg.shape) == (1, 2, 32, 48) and tuple(ver.shape) == (1, 18, 32, 48) and seg.dtype == ver.dtype == torch.bfloat16
    assert seg.untyped_storage().data_ptr() == ver.untyped_storage().data_ptr()   # views of one tensor
    d = worst((seg, ver), ref)
    print(f"{what}, stand-in 1x3x32x48, autocast(bfloat16): eager differs from eager float32 by e = {e:.4e}, fused by {d:.4e} "
          f"({d / e:.2f} e; the bar is 2 e)")
    assert d <= 2 * e
    # float32 features: the wrapped modules (the libraries have one tier) and the float32 tail, under the bar FusedTailNet is held to
    # (the eager float32 network does not reproduce itself bit for bit from call to call -- two calls differ by 1e-7 --, so no equality)
    y32 = torch.cat(fused(x), 1)
    assert y32.dtype == torch.float32 and torch.allclose(y32.double(), ref, atol=1e-5, rtol=1e-5)
    return seg, ver, y32


def hold_forced(case, forced, y32):
    """``precision="bf16"`` on a float32 image: the fused pieces run, float32 out, fewer roundings than under autocast"""
    _, _, x, ref, e = case
    y = torch.cat(forced(x), 1)
    d32 = float((y.double() - ref).abs().max())
    print(f"precision=\"bf16\" on a float32 image: {d32:.4e} = {d32 / e:.2f} e")
    assert y.dtype == torch.float32 and not torch.equal(y, y32) and d32 <= 2 * e


def test_fused_tail_net_against_the_eager_standin_and_into_the_voting_layer(case):
    from pvnet_amd import tail as T, voting
    from tests.test_tail_device import PRECISIONS, hold_stages
    N, net = case[:2]
    x = torch.randn(2, 3, 64, 96, generator=torch.Generator().manual_seed(60)).to(dev())   # two items, more than one block
    with torch.no_grad():
        ref = torch.cat(net(x), 1).cpu()
    fused = N.FusedTailNet(net)
    seg, ver = fused(x)
    torch.cuda.synchronize()
    assert tuple(seg.shape) == (2, 2, 64, 96) and tuple(ver.shape) == (2, 18, 64, 96) and seg.dtype == torch.float32
    assert seg.untyped_storage().data_ptr() == ver.untyped_storage().data_ptr()   # views of one tensor
    assert torch.allclose(torch.cat([seg, ver], 1).cpu(), ref, atol=1e-5, rtol=1e-5)   # float32 features: the float32 tier, G9's bar
    # stage for stage on the features the trunk produced, both tiers
    with torch.no_grad():
        fm = fused._features(x)
    params = (fused.params.w1, fused.params.b1, fused.params.w2, fused.params.b2)
    for precision in PRECISIONS:
        hold_stages(T, fm.cpu(), x.cpu(), params, precision, fm_dev=fm, image_dev=x)
    # the bfloat16 tier against the eager float32 network under the a-priori bound
    seg_b, ver_b = N.FusedTailNet(net, precision="bf16")(x)
    bound, _ = TR.bf16_bound(fm.cpu(), x.cpu(), *params)
    yb = torch.cat([seg_b, ver_b], 1).cpu().double().numpy()
    assert (np.abs(yb - ref.double().numpy()) <= bound + 1e-5 + 1e-5 * np.abs(ref.double().numpy())).all()
    # under autocast the trunk hands over bfloat16 features: the bfloat16 tier, bfloat16 outputs, still views
    seg_a, ver_a = autocast(fused, x)
    assert seg_a.dtype == ver_a.dtype == torch.bfloat16 and not ver_a.is_contiguous()
    # the views go straight into the voting layer: the key-points equal those from contiguous clones
    field = ver_a.permute(0, 2, 3, 1).view(2, 64, 96, 9, 2)
    kp = voting.ransac_voting_layer_v3_from_logits(seg_a, field, 128, inlier_thresh=0.99, seed=3)
    field_c = ver_a.contiguous().permute(0, 2, 3, 1).view(2, 64, 96, 9, 2)
    kp_c = voting.ransac_voting_layer_v3_from_logits(seg_a.contiguous(), field_c, 128, inlier_thresh=0.99, seed=3)
    torch.cuda.synchronize()
    assert tuple(kp.shape) == (2, 9, 2) and torch.equal(kp, kp_c)
    kp_w = voting.EvalWrapper(round_hyp_num=128)(seg_a, ver_a)
    assert tuple(kp_w.shape) == (2, 9, 2)


def test_fused_decoder_net_against_the_eager_standin_and_into_the_voting_layer(case):
    from pvnet_amd import decoder as D, voting
    N, net, x, ref, e = case
    seg, ver, y32 = hold(case, N.FusedDecoderNet(net, stages=D.STAGES), "FusedDecoderNet")
    for stages in (("conv4s",), ("conv2s",), D.DEFAULT_STAGES):   # a stage not named runs its own modules
        assert worst(autocast(N.FusedDecoderNet(net, stages=stages), x), ref) <= 2 * e, stages
    hold_forced(case, N.FusedDecoderNet(net, stages=D.STAGES, precision="bf16"), y32)
    # the views go into the voting layer unchanged
    kp = voting.EvalWrapper(round_hyp_num=128)(seg, ver)
    torch.cuda.synchronize()
    assert tuple(kp.shape) == (1, 9, 2)


def test_fused_stem_net_against_the_eager_standin_and_into_the_voting_layer(case):
    from pvnet_amd import decoder as D, voting
    N, net, x, ref, e = case
    fused = N.FusedStemNet(net, stem=True, stages=D.STAGES)
    seg, ver, y32 = hold(case, fused, "FusedStemNet")
    # the fused stem did run, and its x2s is bfloat16 as the eager stem's under autocast
    assert fused._stem_dtype(x) is None
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        assert fused._stem_dtype(x) == torch.bfloat16
        _, _, x2s = fused._trunk(x)
        x2s_eager = net.stem(x)
    assert x2s.dtype == x2s_eager.dtype == torch.bfloat16 and x2s.shape == x2s_eager.shape and not torch.equal(x2s, x2s_eager)
    hold_forced(case, N.FusedStemNet(net, stem=True, stages=D.STAGES, precision="bf16"), y32)
    # the views go into the voting layer unchanged
    kp = voting.ransac_voting_layer_v3_from_logits(seg, voting._field_view(ver), 128, inlier_thresh=0.99)
    torch.cuda.synchronize()
    assert tuple(kp.shape) == (1, 9, 2)


def test_fused_trunk_net_against_the_eager_standin_and_into_the_voting_layer(case):
    from pvnet_amd import decoder as D, trunk as T, voting
    N, net, x, ref, e = case
    seg, ver, _ = hold(case, N.FusedTrunkNet(net, layers=T.LAYERS, stem=True, stages=D.STAGES), "FusedTrunkNet, all six pieces")
    plain = autocast(N.FusedStemNet(net, stages=D.STAGES), x)
    assert not torch.equal(seg, plain[0])                                         # the fused pieces did run
    # each piece alone stays under the bar too, and a piece not named runs its modules
    for name in T.LAYERS:
        assert worst(autocast(N.FusedTrunkNet(net, layers=(name,), stages=D.STAGES), x), ref) <= 2 * e, name
    with pytest.raises(ValueError):
        N.FusedTrunkNet(net, layers=("layer5",))
    # the views go into the voting layer unchanged
    kp = voting.ransac_voting_layer_v3_from_logits(seg, voting._field_view(ver), 128, inlier_thresh=0.99)
    torch.cuda.synchronize()
    assert tuple(kp.shape) == (1, 9, 2)


def test_a_preset_with_nothing_more_named_is_the_preset_below_it_bit_for_bit(case):
    """The same modules in the same order, then the same launches (tests/test_net_cpu.py holds the order of the calls).  The wrapped
    modules are the convolution library's, whose default choice for two of the stand-in's bfloat16 convolutions at this size
    (l2[0].c2, l3[1].c2) does not return the same bits from one call to the next; asked for deterministic algorithms it does, and only
    then is any network equal to itself, let alone to another."""
    from pvnet_amd import decoder as D
    N, net, x = case[:3]
    none = N.FusedTrunkNet(net, layers=(), stages=D.STAGES)
    assert len(none.blocks) == 0 and none.fc_params is None and none.conv8s_params is None
    pairs = {"FusedTrunkNet(layers=()) is FusedStemNet": (none, N.FusedStemNet(net, stages=D.STAGES)),
             "FusedStemNet(stem=False) is FusedDecoderNet": (N.FusedStemNet(net, stem=False), N.FusedDecoderNet(net)),
             "FusedDecoderNet(stages=()) is FusedTailNet": (N.FusedDecoderNet(net, stages=()), N.FusedTailNet(net))}
    was = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        for what, (one, other) in pairs.items():
            a, b_ = autocast(one, x), autocast(other, x)
            assert a[0].dtype == b_[0].dtype == torch.bfloat16 and torch.equal(a[0], b_[0]) and torch.equal(a[1], b_[1]), what
    finally:
        torch.backends.cudnn.deterministic = was
