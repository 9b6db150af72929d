"""The device pose solve (pnp.pnp_batch_device, pvnet_amd/csrc/pose_solve.hip) against the host library's pnp_batch on the same
float64 problems, at b = 1, 8, 32 and 256: 9 key-points, rotations up to 2.8 rad, 0.4 px noise (tests/test_pose_device.py).

    python tools/pose_probe.py [--reps N]            (needs an MI355X)
    rocprofv3 --kernel-trace --stats -d DIR -o probe -- python tools/pose_probe.py

device: hipEvent time of `reps` back-to-back solves on one stream, divided by reps (warmed up; key-points already on the device);
host:   pnp_batch wall time per call (key-points already on the host -- the copy and sync a real pipeline adds are not counted);
host + round trip: device key-points -> .cpu() -> pnp_batch -> poses back to the device, per call.
Also prints the largest |device - host| pose entry of each size and the mean LM iterations."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pvnet_amd import pnp as P  # noqa: E402


def problems(n, seed=11, pn=9):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-0.08, 0.08, size=(pn, 3))
    x2 = []
    for _ in range(n):
        r = rng.normal(size=3)
        r *= rng.uniform(0.1, 2.8) / np.linalg.norm(r)
        pose = np.concatenate([P.rodrigues(r), np.array([[rng.uniform(-0.2, 0.2)], [rng.uniform(-0.2, 0.2)],
                                                         [rng.uniform(0.5, 1.5)]])], 1)
        x2.append(P.project(X, pose, P.LINEMOD_K) + rng.normal(size=(pn, 2)) * 0.4)
    return X, np.stack(x2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    print("b     device solve (ms)   host pnp_batch (ms)   host + round trip (ms)   max |dev - host|   mean LM iterations")
    for b in (1, 8, 32, 256):
        X, x2 = problems(b)
        Xd, Kd = torch.from_numpy(X).to(dev), torch.from_numpy(P.LINEMOD_K.copy()).to(dev)
        kd = torch.from_numpy(x2).to(dev)
        poses = torch.empty((b, 3, 4), dtype=torch.float64, device=dev)
        status = torch.empty((b,), dtype=torch.int32, device=dev)
        for _ in range(5):
            P.pnp_batch_device(Xd, kd, Kd, out=(poses, status))
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            P.pnp_batch_device(Xd, kd, Kd, out=(poses, status))
        e1.record()
        torch.cuda.synchronize()
        t_dev = e0.elapsed_time(e1) / a.reps
        for _ in range(3):
            want = P.pnp_batch(X, x2, P.LINEMOD_K)
        t0 = time.perf_counter()
        for _ in range(a.reps):
            want = P.pnp_batch(X, x2, P.LINEMOD_K)
        t_host = (time.perf_counter() - t0) / a.reps * 1e3
        t0 = time.perf_counter()
        for _ in range(a.reps):
            back = torch.from_numpy(P.pnp_batch(X, kd.cpu().numpy(), P.LINEMOD_K)).to(dev)
        torch.cuda.synchronize()
        t_rt = (time.perf_counter() - t0) / a.reps * 1e3
        err = float(np.abs(poses.cpu().numpy() - want).max())
        assert back.shape == poses.shape
        print(f"{b:<5d} {t_dev:17.4f}   {t_host:19.4f}   {t_rt:22.4f}   {err:16.2e}   {status.float().mean().item():18.1f}",
              flush=True)


if __name__ == "__main__":
    main()
