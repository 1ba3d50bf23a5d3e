"""Device time of ops.depth_to_points (csrc/frame.hip) on 530 x 730 frames at B = 1 (the live-camera case) and B = 8.

Device events around the operator (both launches), best of --reps, after upload and a warm-up call; readings of
0.4 .. 9.5 m with a tenth of the pixels without depth.  Next to each time the shape-derived bound: 5 B read per pixel
(2 B depth + 3 B colour) plus 24 B written per valid pixel, at --bw TB/s (the measured copy rate).  Prints one JSON
line; --out also writes it to a file."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W = 530, 730


def measure(B, reps, bw):
    from demf_amd import ops
    rng = np.random.default_rng(B)
    mm = rng.integers(400, 9500, size=(B, H, W)).astype(np.uint32)
    mm[rng.random((B, H, W)) < 0.1] = 0
    depth = (((mm << 3) | (mm >> 13)) & 0xFFFF).astype(np.uint16)          # stored rotated left by 3
    rgb = rng.integers(0, 256, size=(B, H, W, 3), dtype=np.uint8)
    tilt = 0.2
    row = [529.5, 529.5, 365.0, 265.0, 1, 0, 0, 0, np.cos(tilt), -np.sin(tilt), 0, np.sin(tilt), np.cos(tilt),
           0.0, 1000.0, 8.0]                                              # pixel_origin, depth_scale, z_max
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()        # noqa: E731
    args = (up(depth.reshape(-1)), up(np.arange(B + 1, dtype=np.int64) * H * W), up(rgb.reshape(-1)),
            up(np.arange(B + 1, dtype=np.int64) * H * W * 3), up(np.array([[H, W, H, W]] * B, np.int32)),
            up(np.array([row] * B, np.float64)))
    raw, off = ops.depth_to_points(*args)
    torch.cuda.synchronize()
    valid = int(off[-1])
    assert valid == int((mm != 0).sum())
    best = float("inf")
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ops.depth_to_points(*args, out=raw)
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1))
    nbytes = 5 * B * H * W + 24 * valid
    bound_us = nbytes / (bw * 1e12) * 1e6
    return dict(B=B, pixels=B * H * W, valid=valid, tiles=-(-B * H * W // ops.FRAME_TILE), us=round(best * 1e3, 2),
                bytes=nbytes, bound_us=round(bound_us, 2), fraction_of_bound=round(bound_us / (best * 1e3), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--bw", type=float, default=6.29, help="copy rate in TB/s the bound is taken at")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = dict(kernel="depth_to_points", frame=[H, W], reps=a.reps, bw_tb_s=a.bw,
               results=[measure(B, a.reps, a.bw) for B in (1, 8)])
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
