"""pvnet_amd -- MI355X-native (gfx950) implementation of PVNet's RANSAC voting hot path.

Public surface (mirrors lib/ransac_voting_gpu_layer of zju3dv/pvnet):
    ransac_voting_layer_v3, generate_hypothesis, voting_for_hypothesis      (pvnet_amd.voting)
    sharded_ransac_voting_layer_v3                                          (pvnet_amd.distributed)
The compute lives in libpvnet_vote.so (HIP, C ABI in include/pvnet_vote.h); build it with
`python -m pvnet_amd.build`.
"""
from .voting import (estimate_voting_distribution_with_mean, generate_hypothesis,  # noqa: F401
                     generate_hypothesis_counts, load_library, ransac_motion_voting, ransac_voting_layer_v3,
                     ransac_voting_layer_v5, voting_for_hypothesis)

_TEXTURE = ("TexturedMeshes", "render_textured", "read_textured_ply", "texture_workspace_bytes")   # pvnet_amd.texture, on first use
_TAIL = ("TailParams", "fused_tail", "FusedTailNet")   # pvnet_amd.tail, on first use
_DECODER = ("StageParams", "fused_stage", "FusedDecoderNet")   # pvnet_amd.decoder, on first use
_STEM = ("StemParams", "fused_stem", "FusedStemNet")   # pvnet_amd.stem, on first use
_TRUNK = ("ConvParams", "fused_conv3x3", "FusedBasicBlock", "FusedTrunkNet")   # pvnet_amd.trunk, on first use
_POSES = {"pnp_classes_device": "pnp", "MultiPoseEvalWrapper": "voting"}   # one pose per (image, class) behind the per-class vote, on first use
_NET = ("FusedNet",)   # pvnet_amd.net, on first use: the network class the four Fused*Net names are presets of

__all__ = ["ransac_voting_layer_v3", "generate_hypothesis", "voting_for_hypothesis", "load_library", *_TEXTURE, *_TAIL, *_DECODER, *_STEM,
           *_TRUNK, *_NET, *_POSES]


def __getattr__(name):
    if name in _TEXTURE:
        from . import texture
        return getattr(texture, name)
    if name in _TAIL:
        from . import tail
        return getattr(tail, name)
    if name in _DECODER:
        from . import decoder
        return getattr(decoder, name)
    if name in _STEM:
        from . import stem
        return getattr(stem, name)
    if name in _TRUNK:
        from . import trunk
        return getattr(trunk, name)
    if name in _POSES:
        import importlib
        return getattr(importlib.import_module("." + _POSES[name], __name__), name)
    if name in _NET:
        from . import net
        return getattr(net, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
