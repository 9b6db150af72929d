"""Regenerates tests/golden/stem.npz.  Run from the repo root where the reference tree is present:  python tests/golden/make_stem_golden.py

stem.npz -- the reference's OWN stem and pool: ``Resnet18_8s.resnet18_8s`` (lib/networks/model_repository.py, lib/networks/resnet.py, no
download) with the seeded stand-in's weights copied in, as fixture G9 is made (tests/golden/make_golden.py), run on the seeded input of
tests/stem_cases.py (1 x 3 x 37 x 53: odd sides).  Recorded: ``x2s`` = relu(bn1(conv1(x))) [1,64,19,27] and ``pooled`` =
maxpool(x2s) [1,64,10,14], float32.
"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = os.environ.get("PVNET_REFERENCE", "/root/reference")
OUT = os.path.join(ROOT, "tests", "golden", "stem.npz")

SCRIPT = r"""
import sys, numpy as np, torch
sys.path.insert(0, %(tools)r); sys.path.insert(0, %(root)r)
import refshim
refshim.install(%(ref)r)
from tests import stem_cases as SC
mine, _ = SC.standin()
x = SC.fixture_input()
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
    x2s = ref.resnet18_8s(x)[0]
    pooled = ref.resnet18_8s.maxpool(x2s)
assert tuple(x2s.shape) == (1, 64, 19, 27) and tuple(pooled.shape) == (1, 64, 10, 14)
np.savez(%(out)r, x2s=x2s.numpy(), pooled=pooled.numpy())
"""


if __name__ == "__main__":
    assert os.path.isdir(REF), "the reference tree is needed"
    code = SCRIPT % dict(tools=os.path.join(ROOT, "tools"), root=ROOT, ref=REF, out=OUT)
    subprocess.check_call([sys.executable, "-B", "-c", code], cwd=ROOT)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")
