"""The device pose metrics (evaluation.pose_metrics_device, pvnet_amd/csrc/pose_metrics.hip) against the host Evaluator._record loop
on the same poses: b = 1, 8, 32, 256 images of one class; model sizes 1 000 / 5 000 / 20 000 points; a plain class ('cat': ADD,
projection) and a symmetric one ('eggbox': ADD-S, and with --sym-projection also the symmetric projection error).

    python tools/metrics_probe.py [--reps N] [--host-reps N] [--sym-projection]      (needs an MI355X)
    rocprofv3 --kernel-trace --stats -d DIR -o probe -- python tools/metrics_probe.py

device: hipEvent time of `reps` back-to-back calls on one stream, divided by reps (warmed up; poses already on the device;
        caller-owned outputs and workspace);
host:   Evaluator._record per image, summed over the batch (poses already on the host; its symmetric search runs pvnet_nn on the
        GPU with a copy there and back per image).  Measured on the first `host-reps` batches of a size only.
For symmetric rows also the search's rate: pair tests per second (b x m^2 per search) and its share of the 157.3 TFLOP/s FP32
vector peak, counting 8 flops per 3-D test (3 sub, 3 mul, 2 add)."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pvnet_amd import evaluation as E  # noqa: E402
from pvnet_amd import pnp as P  # noqa: E402

PEAK_FP32 = 157.3e12


def poses(rng, b):
    tg, pr = [], []
    for _ in range(b):
        r = rng.normal(size=3)
        r *= rng.uniform(0.0, np.pi) / np.linalg.norm(r)
        t = np.array([rng.uniform(-0.2, 0.2), rng.uniform(-0.2, 0.2), rng.uniform(0.6, 1.5)])
        T = np.concatenate([P.rodrigues(r), t[:, None]], 1)
        d = rng.normal(size=3)
        d *= np.deg2rad(rng.uniform(0, 8)) / np.linalg.norm(d)
        Pp = T.copy()
        Pp[:, :3] = P.rodrigues(d) @ T[:, :3]
        Pp[:, 3] += rng.normal(size=3) * 0.02
        tg.append(T)
        pr.append(Pp)
    return np.stack(pr), np.stack(tg)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--sym-projection", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    K = P.LINEMOD_K
    print(f"sym_projection={a.sym_projection}")
    print("class   points     b   device (ms)   host loop (ms)   host/device   search pair tests/s   share of FP32 peak")
    for npts in (1000, 5000, 20000):
        model = rng.uniform(-0.1, 0.1, (npts, 3))
        models = {"cat": model, "eggbox": model}
        diam = {"cat": 0.25, "eggbox": 0.25}
        dm = E.DeviceModels(models, diam, dev)
        Kd = torch.from_numpy(K.copy()).to(dev)
        ev = E.Evaluator(models=models, diameters=diam)
        for cls in ("cat", "eggbox"):
            for b in (1, 8, 32, 256):
                pr, tg = poses(rng, b)
                prd, tgd = torch.from_numpy(pr).to(dev), torch.from_numpy(tg).to(dev)
                ids = torch.full((b,), dm.index(cls), dtype=torch.int32, device=dev)
                out = (torch.empty((b, 4), dtype=torch.float64, device=dev), torch.empty((b, 3), dtype=torch.bool, device=dev),
                       torch.empty((b,), dtype=torch.int32, device=dev))
                ws = torch.empty(E.pose_metrics_workspace_bytes(b, dm, a.sym_projection), dtype=torch.uint8, device=dev)

                def call():
                    E.pose_metrics_device(prd, tgd, Kd, dm, class_ids=ids, sym_projection=a.sym_projection, out=out, workspace=ws)

                for _ in range(5):
                    call()
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.reps):
                    call()
                e1.record()
                torch.cuda.synchronize()
                t_dev = e0.elapsed_time(e1) / a.reps
                # host loop: skipped where it would take minutes (symmetric 20 000-point models at b = 256)
                hb = b if not (cls == "eggbox" and npts * b > 2_000_000) else max(1, 2_000_000 // npts)
                ev._record(pr[0], tg[0], cls, K, sym_projection=a.sym_projection)   # warm
                t0 = time.perf_counter()
                for _ in range(a.host_reps):
                    for i in range(hb):
                        ev._record(pr[i], tg[i], cls, K, sym_projection=a.sym_projection)
                t_host = (time.perf_counter() - t0) * 1e3 / a.host_reps * b / hb
                note = "" if hb == b else f" (x{b / hb:.0f} from b={hb})"
                if cls == "eggbox":
                    searches = 2 if a.sym_projection else 1
                    tests = b * npts * npts * searches
                    rate = tests / (t_dev * 1e-3)
                    extra = f"{rate:18.3e}   {rate * 8 / PEAK_FP32 * 100:14.1f} %"
                else:
                    extra = ""
                print(f"{cls:7s} {npts:6d} {b:5d} {t_dev:12.4f} {t_host:15.2f}{note} {t_host / t_dev:12.1f}   {extra}", flush=True)


if __name__ == "__main__":
    main()
