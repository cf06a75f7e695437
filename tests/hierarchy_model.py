"""Hierarchy simplification restated in numpy: the contract of pcpx_hierarchy_simplification (include/pcpx.h, DESIGN.md
section 14), and a float32 restatement of the reference's queue (include/pcp/algorithm/hierarchy_simplification.hpp:63-149)
to measure how far the contract's float64 decisions move the result.

`hierarchy(points, cluster_size, var_max)` runs level by level, vectorised (np.add.reduceat over the clusters' ranges,
one batched eigh per level), so clouds of 10^6 points take seconds.  Besides the kept input indices it returns the
decision margins, each the minimum over every decision of its kind, so a test can state how close a case comes to a
decision that rounding could flip:
  f      |p.n - d| / r over the points of every cluster that wants a split (r: the cluster's largest distance to its mean)
  var    |var - (float)var_max| over the clusters whose size does not force a split
  gap    (l2 - l1) / l2 over the clusters that want a split (the eigenvector n is only determined up to this)
  sign   (|n|_1st - |n|_2nd) / |n|_1st where n's two largest-magnitude components have opposite signs (the sign rule)
  d2     (second - best) / second squared distance to the mean in every leaf, exact duplicates of the best point excluded;
         leaves of two points are exact ties by symmetry and not counted: their mean is the correctly rounded (a + b) / 2
         in any summation order, so every implementation computes the same two distances and takes the smaller index
"""
import numpy as np

MARGINS = ("f", "var", "gap", "sign", "d2")


def _seg_min(a, starts):
    return np.minimum.reduceat(a, starts) if len(a) else a


def hierarchy(points, cluster_size, var_max=1.0 / 3.0):
    """-> dict(idx: kept input indices (uint32) in queue order, margins: {name: float}, levels: int)."""
    P = np.ascontiguousarray(points, np.float32).reshape(-1, 3).astype(np.float64)
    n = len(P)
    vmax = float(np.float32(var_max))
    margins = {m: np.inf for m in MARGINS}
    out = []
    perm = np.arange(n, dtype=np.int64)  # the active points, cluster after cluster, input order inside each
    counts = np.array([n], np.int64) if n else np.zeros(0, np.int64)
    levels = 0
    while len(counts):
        levels += 1
        K = len(counts)
        starts = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64)
        seg = np.repeat(np.arange(K), counts)
        X = P[perm]
        mu = np.add.reduceat(X, starts, axis=0) / counts[:, None]
        D = X - mu[seg]
        dx, dy, dz = D[:, 0], D[:, 1], D[:, 2]
        xx, xy, xz = (np.add.reduceat(v, starts) for v in (dx * dx, dx * dy, dx * dz))
        yy, yz, zz = (np.add.reduceat(v, starts) for v in (dy * dy, dy * dz, dz * dz))
        A = np.stack([np.stack([xx, xy, xz], 1), np.stack([xy, yy, yz], 1), np.stack([xz, yz, zz], 1)], 1)
        w, V = np.linalg.eigh(A)
        with np.errstate(invalid="ignore", divide="ignore"):
            var = w[:, 0] / (w[:, 0] + w[:, 1] + w[:, 2])
        wants = (counts > cluster_size) | (var > vmax)
        nv = V[:, :, 2]
        big = np.argmax(np.abs(nv), axis=1)
        flip = nv[np.arange(K), big] < 0
        nv = np.where(flip[:, None], -nv, nv)
        d = mu[:, 0] * nv[:, 0] + mu[:, 1] * nv[:, 1] + mu[:, 2] * nv[:, 2]
        ns = nv[seg]
        f = X[:, 0] * ns[:, 0] + X[:, 1] * ns[:, 1] + X[:, 2] * ns[:, 2] - d[seg]
        left = (f <= 0.0) & wants[seg]
        nl = np.add.reduceat(left.astype(np.int64), starts)
        split = wants & (nl > 0) & (nl < counts)
        d2 = dx * dx + dy * dy + dz * dz
        best = _seg_min(d2, starts)
        pos = np.arange(len(perm), dtype=np.int64)
        first = _seg_min(np.where(d2 == best[seg], pos, len(perm)), starts)  # smallest position = smallest input index
        leaf = ~split
        out.append(perm[first[leaf]])

        # margins
        r = np.sqrt(np.maximum.reduceat(d2, starts))
        spread = wants & (r > 0)
        sel = spread[seg]
        if sel.any():
            margins["f"] = min(margins["f"], float(np.min(np.abs(f[sel]) / r[seg][sel])))
            margins["gap"] = min(margins["gap"], float(np.min((w[spread, 2] - w[spread, 1]) / w[spread, 2])))
            a = np.sort(np.abs(nv[spread]), axis=1)
            order = np.argsort(-np.abs(nv[spread]), axis=1, kind="stable")
            s1 = np.take_along_axis(nv[spread], order[:, :1], 1)[:, 0]
            s2 = np.take_along_axis(nv[spread], order[:, 1:2], 1)[:, 0]
            opp = (s1 * s2) < 0
            if opp.any():
                margins["sign"] = min(margins["sign"], float(np.min(((a[:, 2] - a[:, 1]) / a[:, 2])[opp])))
        decides = (counts <= cluster_size) & ~np.isnan(var)
        if decides.any():
            margins["var"] = min(margins["var"], float(np.min(np.abs(var[decides] - vmax))))
        if leaf.any():
            bp = X[first][seg]
            dup = np.all(X == bp, axis=1)
            second = _seg_min(np.where(dup, np.inf, d2), starts)
            ok = leaf & np.isfinite(second) & (counts > 2)
            if ok.any():
                margins["d2"] = min(margins["d2"], float(np.min((second[ok] - best[ok]) / second[ok])))

        # children: the split clusters' points, stably partitioned (left first)
        keep = split[seg]
        key = seg * 2 + (~left).astype(np.int64)
        sub = np.nonzero(keep)[0]
        perm = perm[sub[np.argsort(key[sub], kind="stable")]]
        counts = np.stack([nl[split], counts[split] - nl[split]], 1).ravel()
    idx = np.concatenate(out).astype(np.uint32) if out else np.zeros(0, np.uint32)
    return {"idx": idx, "margins": margins, "levels": levels}


def reference_float32(points, cluster_size, var_max=1.0 / 3.0):
    """The reference's queue in float32: sequential float sums (center_of_geometry, covariance.hpp:61-89), eigh of the
    float32 scatter (Eigen's solver is not available here: float64 eigh rounded to float32), var and the plane test in
    float32, libstdc++'s bidirectional std::partition (swaps, unstable) and std::min_element (first strict minimum).
    Returns the kept input indices in queue order.  Slow: a Python loop over clusters."""
    P = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    F = np.float32
    vmax = F(var_max)
    idx = np.arange(len(P), dtype=np.int64)
    queue = [(0, len(P))] if len(P) else []
    out = []
    head = 0
    while head < len(queue):
        b, e = queue[head]
        head += 1
        X = P[idx[b:e]]
        N = e - b
        s = np.cumsum(X, axis=0, dtype=np.float32)[-1]  # sequential float sums
        mu = (s / F(N)).astype(np.float32)
        D = (X - mu).astype(np.float32)
        prods = np.stack([D[:, 0] * D[:, 0], D[:, 1] * D[:, 1], D[:, 2] * D[:, 2], D[:, 0] * D[:, 1], D[:, 0] * D[:, 2],
                          D[:, 1] * D[:, 2]], 1).astype(np.float32)
        c = np.cumsum(prods, axis=0, dtype=np.float32)[-1]
        A = np.array([[c[0], c[3], c[4]], [c[3], c[1], c[5]], [c[4], c[5], c[2]]], np.float64)
        w, V = np.linalg.eigh(A)
        w = w.astype(np.float32)
        with np.errstate(invalid="ignore", divide="ignore"):
            var = F(w[0] / F(F(w[0] + w[1]) + w[2]))
        if N > cluster_size or var > vmax:
            nv = V[:, 2].astype(np.float32)
            d = F(F(F(mu[0] * nv[0]) + F(mu[1] * nv[1])) + F(mu[2] * nv[2]))
            f = ((X[:, 0] * nv[0] + X[:, 1] * nv[1]).astype(np.float32) + X[:, 2] * nv[2]).astype(np.float32) - d
            pred = list(f <= F(0))
            sub = list(idx[b:e])
            first, last = 0, N  # libstdc++ __partition, bidirectional form
            while True:
                while first != last and pred[first]:
                    first += 1
                if first == last:
                    break
                last -= 1
                while first != last and not pred[last]:
                    last -= 1
                if first == last:
                    break
                sub[first], sub[last] = sub[last], sub[first]
                pred[first], pred[last] = pred[last], pred[first]
                first += 1
            idx[b:e] = sub
            if first == 0 or first == N:  # the reference loops forever here; the contract's leaf rule
                queue_leaf = True
            else:
                queue_leaf = False
                queue.append((b, b + first))
                queue.append((b + first, e))
            if not queue_leaf:
                continue
            X = P[idx[b:e]]
            D = (X - mu).astype(np.float32)
        d2 = ((D[:, 0] * D[:, 0] + D[:, 1] * D[:, 1]).astype(np.float32) + D[:, 2] * D[:, 2]).astype(np.float32)
        out.append(idx[b + int(np.argmin(d2))])
    return np.array(out, np.uint32)
