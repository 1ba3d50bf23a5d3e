"""Seeded boxes for the NMS and merge tests, filtered on the CPU by decision margin before either side runs.

Not a test module.  A scene of clustered detections: base boxes uniform in a +-``half`` m square (4 m unless a test
asks for a sparser scene), sizes 0.3 - 2 m, any yaw; every base box is repeated ``DUP`` = 4 times with centre
jitter sigma 0.05 m, size factor 0.9 - 1.1 and yaw jitter sigma 0.05 - what the views of a scene hand the merge.

Decision margin.  A flipped ``iou > thr`` decision cascades through a greedy NMS, so a case must not hold a pair
whose IoU the fp32 kernel and the fp64 reference may place on different sides of ``thr``.  The margin is the
project's own 1e-4 (tests/test_gpu_eval.py: an fp32 IoU that agrees with fp64 to 1e-5): about 10 % more boxes than
needed are generated, a box whose fp64 IoU with an earlier box that stays lies within the margin of ``thr`` is
dropped, and the rest is truncated to exactly ``n``.  The filter may drop at most 3 % of the generated boxes
(``filtered`` asserts it): it removes a few knife-edge pairs, it does not shape the case.  Nothing is dropped after
the GPU has run.
"""
import functools

import numpy as np

import tta_reference as tref

DUP = 4
MARGIN = 1e-4
MAX_DROP = 0.03


def raw(seed, m, half=4.0):
    """m clustered boxes (m,7) fp32 bottom-centre and distinct scores (m,) fp32, in a seeded random order."""
    rng = np.random.default_rng([int(seed), int(m)])
    nb = -(-m // DUP)
    base = np.concatenate([rng.uniform(-half, half, (nb, 2)), rng.uniform(0.0, 1.0, (nb, 1)),
                           rng.uniform(0.3, 2.0, (nb, 3)), rng.uniform(-np.pi, np.pi, (nb, 1))], 1)
    b = np.repeat(base, DUP, 0)
    b[:, :3] += rng.normal(scale=0.05, size=(len(b), 3))
    b[:, 3:6] *= rng.uniform(0.9, 1.1, (len(b), 3))
    b[:, 6] += rng.normal(scale=0.05, size=len(b))
    b = b[rng.permutation(len(b))[:m]]
    scores = rng.permutation(np.linspace(0.05, 0.95, m)).astype(np.float32)
    assert len(np.unique(scores)) == m
    return b.astype(np.float32), scores


@functools.lru_cache(maxsize=None)
def filtered(seed, n, thr, mode="bev", half=4.0):
    """-> (boxes (n,7) fp32, scores (n,) fp32, ious (n,n) float64 of those boxes under ``mode``)."""
    if n == 0:
        return np.zeros((0, 7), np.float32), np.zeros((0,), np.float32), np.zeros((0, 0))
    m = n + max(2, -(-n // 10))
    boxes, scores = raw(seed, m, half)
    ious = tref.iou_matrix(boxes, mode)
    edge = np.abs(ious - thr) < MARGIN
    stay = []
    for j in range(m):
        if not edge[j, stay].any():
            stay.append(j)
    dropped = m - len(stay)
    assert dropped <= MAX_DROP * m, f"the margin filter dropped {dropped} of {m} boxes"
    assert len(stay) >= n
    stay = np.asarray(stay[:n])
    return boxes[stay], scores[stay], ious[np.ix_(stay, stay)]
