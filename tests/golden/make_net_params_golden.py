"""Regenerates tests/golden/net_params_parent.json: SHA-256 digests of every tensor the four parameter classes of the fused network
build from the seeded stand-in (tests/tail_cases.py), through the public classes only.  It was run at the commit before the wrappers'
plumbing moved into pvnet_amd/_net.py, so the file records that commit's bits; tests/test_net_common_cpu.py holds every later tree to
them.  Run from the repo root:  python tests/golden/make_net_params_golden.py"""
import hashlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "net_params_parent.json")


def digest(t):
    t = t.detach().cpu().contiguous()
    return f"{str(t.dtype).replace('torch.', '')}{list(t.shape)}:" + hashlib.sha256(t.view(torch.uint8).numpy().tobytes()).hexdigest()


def digests():
    """name -> digest, of the stand-in's tail, stages, stem and every convolution of the trunk"""
    from pvnet_amd.decoder import STAGES, StageParams
    from pvnet_amd.stem import StemParams
    from pvnet_amd.tail import TailParams
    from pvnet_amd.trunk import LAYERS, FusedTrunkNet
    from tests import tail_cases, trunk_cases
    out = {}

    def put(prefix, params, names):
        for n in names:
            out[f"{prefix}.{n}"] = digest(getattr(params, n))

    net = tail_cases.standin()[0]
    put("tail", TailParams.from_network(net), ("w1", "b1", "w2", "b2"))
    for stage in STAGES:
        put(stage, StageParams.from_network(net, stage), ("w", "bias", "packed"))
    put("stem", StemParams.from_network(net), ("w", "bias"))
    fused = FusedTrunkNet(trunk_cases.standin(), layers=LAYERS)
    for name in LAYERS[:4]:
        for i, blk in enumerate(fused.blocks[name]):
            put(f"{name}.{i}.conv1", blk.conv1, ("w", "bias", "packed"))
            put(f"{name}.{i}.conv2", blk.conv2, ("w", "bias", "packed"))
            if blk.down is not None:
                out[f"{name}.{i}.down.w"], out[f"{name}.{i}.down.bias"] = (digest(t) for t in blk.down)
    put("fc", fused.fc_params, ("w", "bias", "packed"))
    put("conv8s", fused.conv8s_params, ("w", "bias", "packed"))
    return out


if __name__ == "__main__":
    with open(OUT, "w") as fh:
        json.dump(digests(), fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(OUT)
