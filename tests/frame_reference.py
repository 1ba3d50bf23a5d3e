"""Float64 numpy restatement of the RGB-D frame front end (csrc/frame.hip, include/demf_hip.h demf_depth_to_points)
that tests/test_gpu_frame.py holds the kernel against bit for bit.  Every step is one element-wise IEEE operation in
the order the header states; no ``@`` / ``dot`` (BLAS may fuse and reorder).  Independent of the product code."""
import numpy as np

DEFAULTS = dict(pixel_origin=0.0, depth_scale=1000.0, z_max=8.0)


def rotate_right16(d, shift):
    """uint16 words rotated right by ``shift`` bits."""
    d = np.asarray(d, np.uint16).astype(np.uint32)
    return (((d >> np.uint32(shift)) | (d << np.uint32(16 - shift))) & np.uint32(0xFFFF)).astype(np.uint16)


def calib_row(K, Rt, pixel_origin=0.0, depth_scale=1000.0, z_max=8.0):
    """-> the (16,) fp64 row [fx, fy, cx, cy, Rt row-major (9), pixel_origin, depth_scale, z_max]."""
    K = np.asarray(K, np.float64).reshape(3, 3)
    return np.concatenate([[K[0, 0], K[1, 1], K[0, 2], K[1, 2]], np.asarray(Rt, np.float64).reshape(9),
                           [pixel_origin, depth_scale, z_max]]).astype(np.float64)


def frame_records(depth, rgb, calib, shift=3):
    """One frame: depth (h, w) uint16, rgb (h, w, 3) uint8, calib (16,) fp64 -> the (n_valid, 6) fp32 records of the
    valid pixels in row-major order."""
    depth = np.asarray(depth, np.uint16)
    h, w = depth.shape
    q = np.asarray(calib, np.float64)
    fx, fy, cx, cy = q[0], q[1], q[2], q[3]
    rt = q[4:13].reshape(3, 3)
    origin, scale, z_max = q[13], q[14], q[15]
    d = rotate_right16(depth, shift)
    valid = d != 0
    z = np.minimum(d.astype(np.float64) / scale, z_max)
    v, u = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    x3 = ((u + origin) - cx) * z / fx
    y3 = ((v + origin) - cy) * z / fy
    c = (x3, z, -y3)
    p = [(rt[i, 0] * c[0] + rt[i, 1] * c[1]) + rt[i, 2] * c[2] for i in range(3)]
    col = np.asarray(rgb, np.uint8).reshape(h, w, 3).astype(np.float32) / np.float32(255.0)
    rec = np.stack([p[0].astype(np.float32), p[1].astype(np.float32), p[2].astype(np.float32),
                    col[..., 0], col[..., 1], col[..., 2]], -1)
    return rec[valid].astype(np.float32)


def depth_to_points(depths, rgbs, calibs, shift=3):
    """B frames -> (records (total_valid, 6) fp32, offsets (B+1,) int64): frames in order."""
    recs = [frame_records(d, c, q, shift) for d, c, q in zip(depths, rgbs, calibs)]
    off = np.concatenate([[0], np.cumsum([len(r) for r in recs])]).astype(np.int64)
    return np.concatenate(recs, 0).reshape(-1, 6).astype(np.float32), off
