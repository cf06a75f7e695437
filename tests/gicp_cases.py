"""pcpx_gicp_rigid with PCPX_GICP_ON_DEVICE as rows in the form of tests/exact_buffers_cases.py -- a callable over a Buffers, which
tests/test_gpu_gicp.py runs on plain buffers, on the exact-size buffers of tests/exact_buffers.py and on the held stream of
tests/stream_order.py -- and the inputs they run on: that table's clouds and sources, random unit normals for the source, the
cloud's own for the target, or the covariances those normals stand for.  tests/test_gpu_gicp.py pins the plain form to the host
call and to the model."""
import functools

import numpy as np

import gicp_model as G
import handle_history_cases as HH

F = np.float32
EPSILON = 0.05


@functools.lru_cache(maxsize=None)
def inputs(cloud, by_cov):
    """(by source row, by input row of the target): normals (rows of 3) or covariances (rows of 6)"""
    I = HH.inputs(cloud)
    a, b = HH._unit(np.random.default_rng(HH.SEEDS[cloud] + 1), len(I["source"])), I["normals"]
    out = tuple(G.covariances_of_normals(x, EPSILON).astype(F) for x in (a, b)) if by_cov else (a, b)
    for x in out:
        x.setflags(write=False)
    return out


def row(c, by_cov):
    """gicp_dev over a Buffers (the out / up / ready / drain / down interface of handle_history_cases.Ctx)"""
    s, it = c.I["source"], HH.ICP_ITERATIONS
    m = len(s)
    a, b = inputs(c.cloud, by_cov)
    src, d_a, d_b, xf, words = c.up(s), c.up(a), c.up(b), c.out(16, "f64"), [c.out(1, "u32") for _ in range(3)]
    count, rms, partner = c.out(it, "u32"), c.out(it, "f64"), c.out(m, "u32")
    c.ready()
    kw = dict(d_source_cov=d_a, d_cov=d_b) if by_cov else dict(d_source_normals=d_a, d_normals=d_b, epsilon=EPSILON)
    c.ix.gicp_dev(src, m, 2.0 * c.r, xf, max_iterations=it, d_status=words[0], d_iterations=words[1], d_last_count=words[2], d_count=count, d_rms=rms,
                  d_partner=partner, **kw)
    c.drain()
    return {"transform": c.down(xf, 16), "words": np.concatenate([c.down(w, 1) for w in words]), "count": c.down(count, it), "rms": c.down(rms, it),
            "partner": c.down(partner, m)}
