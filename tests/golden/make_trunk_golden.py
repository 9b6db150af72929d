"""Regenerates tests/golden/trunk.npz.  Run from the repo root where the reference tree is present:  python tests/golden/make_trunk_golden.py

trunk.npz -- the reference's OWN residual trunk: ``Resnet18_8s`` (lib/networks/model_repository.py, lib/networks/resnet.py, no download)
with the seeded stand-in's weights copied in, as fixture G9 is made (tests/golden/make_golden.py), run on the seeded input of
tests/trunk_cases.py (1 x 3 x 64 x 88).  Recorded, float32: ``pooled`` = maxpool(x2s) [1,64,16,22], what layer1 takes; ``x4s``
[1,64,16,22], ``x8s`` [1,128,8,11], ``x16s`` [1,256,8,11], ``x32s`` [1,512,8,11] = the outputs of layer1 .. layer4; ``xfc`` [1,256,8,11];
``conv8s`` = conv8s(cat([xfc, x8s], 1)) [1,128,8,11].
"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = os.environ.get("PVNET_REFERENCE", "/root/reference")
OUT = os.path.join(ROOT, "tests", "golden", "trunk.npz")

SCRIPT = r"""
import sys, numpy as np, torch
sys.path.insert(0, %(tools)r); sys.path.insert(0, %(root)r)
import refshim
refshim.install(%(ref)r)
from tests import trunk_cases as TC
mine = TC.standin()
x = TC.fixture_input()
for k in [k for k in sys.modules if k == "lib" or k.startswith("lib.")]:
    del sys.modules[k]                           # the repo's drop-in overlay package is also called `lib`
sys.path.insert(0, %(ref)r)
import lib.networks.resnet as R
R.model_zoo.load_url = lambda *a, **k: {}        # no network here
R.ResNet.load_state_dict = lambda self, sd, *a, **k: None
from lib.networks.model_repository import Resnet18_8s
ref = Resnet18_8s(ver_dim=18, seg_dim=2).eval()
rp, mp = list(ref.parameters()), list(mine.parameters())
rb, mb = list(ref.buffers()), list(mine.buffers())
assert [p.shape for p in rp] == [p.shape for p in mp] and [b.shape for b in rb] == [b.shape for b in mb]
with torch.no_grad():
    for a, b in zip(rp + rb, mp + mb):
        a.copy_(b)
    x2s, x4s, x8s, x16s, x32s, xfc = ref.resnet18_8s(x)
    pooled = ref.resnet18_8s.maxpool(x2s)
    c8 = ref.conv8s(torch.cat([xfc, x8s], 1))
assert tuple(pooled.shape) == (1, 64, 16, 22) and tuple(x32s.shape) == (1, 512, 8, 11) and tuple(c8.shape) == (1, 128, 8, 11)
np.savez_compressed(%(out)r, pooled=pooled.numpy(), x4s=x4s.numpy(), x8s=x8s.numpy(), x16s=x16s.numpy(), x32s=x32s.numpy(),
                    xfc=xfc.numpy(), conv8s=c8.numpy())
"""


if __name__ == "__main__":
    assert os.path.isdir(REF), "the reference tree is needed"
    code = SCRIPT % dict(tools=os.path.join(ROOT, "tools"), root=ROOT, ref=REF, out=OUT)
    subprocess.check_call([sys.executable, "-B", "-c", code], cwd=ROOT)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")
