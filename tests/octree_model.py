"""OctreeGridDataPointsFilter of the input filter chain (include/lsgpu_icp.h, "the input filter chain"; DESIGN.md §5 choices
49-54): the contract restated as a numpy-float32 recursion, with no call into the library.  The draws of RandomPts are handed
in by the caller.  Every np.float32 operation below rounds once, as the contract asks."""
import numpy as np

F = np.float32
MAX_DEPTH = 21
FIRST_PTS, RANDOM_PTS, CENTROID, MEDOID = 0, 1, 2, 3


class Leaf:
    """One visited leaf: its points' input indices (ascending), depth, radius and why it stopped ('size', 'count', 'depth':
    the first rule that held, in the contract's order)."""
    __slots__ = ("idx", "depth", "radius", "why", "tie")

    def __init__(self, idx, depth, radius, why):
        self.idx, self.depth, self.radius, self.why, self.tie = idx, depth, radius, why, False


def _leaf_point(pts, leaf, method, draw):
    idx = leaf.idx
    if method == FIRST_PTS:
        return pts[idx[0]].copy()
    if method == RANDOM_PTS:
        return pts[idx[int(F(len(idx) - 1) * F(draw))]].copy()
    sub = pts[idx, :3]
    # ufunc.accumulate adds strictly one element after the other (no pairwise blocks): s = p0, s += p1, s += p2, ...
    # (sequential_sum below is the same as a plain loop; tests/test_octree_filter.py compares the two)
    cen = np.add.accumulate(sub, axis=0, dtype=np.float32)[-1] / F(len(idx))
    if method == CENTROID:
        out = pts[idx[0]].copy()                      # (w: the first point's, bits and all)
        out[:3] = cen
        return out
    d = sub - cen                                     # elementwise float32: every operation rounds once
    dist = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    assert dist.dtype == np.float32
    best = int(np.argmin(dist))                       # the first of equal minima: strict <, the earliest wins
    leaf.tie = int((dist == dist[best]).sum()) > 1
    return pts[idx[best]].copy()


def sequential_sum(v):
    """The plain loop the contract states, for one coordinate."""
    s = F(v[0])
    for x in v[1:]:
        s = s + F(x)
    return s


def octree_grid(pts, max_size=0.0, max_point=1, method=FIRST_PTS, draws=None):
    """-> (output points (m, 4) float32, [Leaf] in visiting order).  draws: a sequence of float32, one per leaf (RandomPts)."""
    pts = np.ascontiguousarray(pts, np.float32)
    n = pts.shape[0]
    assert n > 0 and np.isfinite(pts[:, :3]).all()
    max_size = F(max_size)
    lo, hi = pts[:, :3].min(0), pts[:, :3].max(0)
    ext = [hi[a] - lo[a] for a in range(3)]
    center = [lo[a] + ext[a] * F(0.5) for a in range(3)]
    radius = max(ext) * F(0.5)
    leaves = []

    def node(idx, c, r, depth):
        if F(2.0) * r <= max_size:
            leaves.append(Leaf(idx, depth, r, "size"))
            return
        if len(idx) <= max_point:
            leaves.append(Leaf(idx, depth, r, "count"))
            return
        if depth == MAX_DEPTH:
            leaves.append(Leaf(idx, depth, r, "depth"))
            return
        sub = pts[idx]
        octant = (sub[:, 0] > c[0]).astype(np.int64) | ((sub[:, 1] > c[1]).astype(np.int64) << 1) | ((sub[:, 2] > c[2]).astype(np.int64) << 2)
        r2 = r * F(0.5)
        for o in range(8):
            child = idx[octant == o]                  # (a boolean mask keeps ascending input index)
            if child.size == 0:
                continue
            node(child, [c[a] + r2 if (o >> a) & 1 else c[a] - r2 for a in range(3)], r2, depth + 1)

    node(np.arange(n, dtype=np.int64), center, radius, 0)
    out = np.empty((len(leaves), 4), np.float32)
    for k, leaf in enumerate(leaves):
        out[k] = _leaf_point(pts, leaf, method, draws[k] if method == RANDOM_PTS else 0.0)
    return out, leaves
