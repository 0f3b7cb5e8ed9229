"""The forward substitution of a reusing step through the kept x panels in one launch (k_fwd_prefix).

A reusing step sends the new right-hand side through the panels it keeps.  PYIPM_FWD_PREFIX=0 (read when the handle is created)
does that with the per-panel launches -- k_fwd_diag, k_fwd_gemv, k_diag_apply for every kept panel --, otherwise one k_fwd_prefix
launch and one k_diag_apply over the kept tiles do.  Both add the same products in the same order, so every comparison here is
BIT FOR BIT: the direction as int64 patterns and every field of the statistics, over three steps of one handle (a recording one,
two reusing ones) with other s, lambda, mu and another right-hand side each time, and the reuse counter says that steps 1 and 2
did reuse.  A consumer that read the step before's value would show on steps 1 and 2: the vectors of step k + 1 differ from
step k's in every entry (checked on the reference's directions).  All of it in the suite's NaN-filled workspace.
No test here provokes a timeout: the error path of the kernel is reviewed by reading."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

STEPS = 3
# (n, me, mi), nb: N = 1152 (two prefix groups, a slack hole); N = 896 = 7 x 128 rows; panels of four tiles; no slack hole; me = 0
SHAPES = [((512, 128, 256), 128), ((384, 128, 192), 128), ((1024, 256, 512), 256), ((512, 128, 0), 128), ((512, 0, 256), 128)]
IDS = ["n512", "n384_odd_panels", "n1024_nb256", "mi0", "me0"]


def _qp(shape):
    from pyipm_amd.problems import make_qp
    return make_qp(shape[0], shape[1], shape[2], seed=11)


def _vec(qp, k):
    """Vectors of step k: other s, lda, mu and right-hand side each time, every entry another one."""
    n, me, mi = qp["n"], qp["me"], qp["mi"]
    rng = np.random.default_rng(2000 + k)
    return dict(df=qp["df"] + 0.1 * rng.standard_normal(n), ce=qp["ce"] + 0.1 * rng.standard_normal(me),
                ci=qp["ci"] + 0.1 * rng.standard_normal(mi), s=qp["s"] * rng.uniform(0.5, 2.0, mi),
                lda=qp["lam"] * rng.uniform(0.5, 2.0, me + mi), mu=0.3 / (k + 1))


def _core(shape, nb, one_launch, opts=()):
    from pyipm_amd.newton import NewtonCore
    saved = os.environ.get("PYIPM_FWD_PREFIX")
    os.environ["PYIPM_FWD_PREFIX"] = "1" if one_launch else "0"          # (read when the handle is created)
    try:
        core = NewtonCore(shape[0], shape[1], shape[2], device=0, nb=nb)
    finally:
        if saved is None:
            os.environ.pop("PYIPM_FWD_PREFIX")
        else:
            os.environ["PYIPM_FWD_PREFIX"] = saved
    core.set_option("expert", 1)
    core.set_option("group", 2)
    for k, v in opts:                   # (before the first step: any set_option call drops a recorded prefix)
        core.set_option(k, v)
    return core


def _run(shape, nb, one_launch, opts=()):
    """STEPS steps of one handle: [(dz bits, statistics)], each step checked to be of the kind it is meant to be."""
    import torch
    assert os.environ.get("PYIPM_POISON_WORKSPACE")
    qp = _qp(shape)
    core = _core(shape, nb, one_launch, opts)
    core.stage_blocks(qp["d2L"], qp["Je"], qp["Ji"])
    out = []
    for k in range(STEPS):
        v = _vec(qp, k)
        core.stage_vectors(v["df"], v["ce"], v["ci"], v["s"], v["lda"], mu=v["mu"])
        dz, st = core.step(0.0, 0.0, 0)
        info = core.reuse_info()
        assert info["reused"] == k and info["last"] == ("recording" if k == 0 else "reusing"), (shape, k, info)
        out.append((dz.clone().view(torch.int64), st))
    core.close()
    return out


_REF = {}


def _ref(shape, nb, opts=()):
    """The per-panel forward substitution (PYIPM_FWD_PREFIX=0) under the same options: computed once per key, never changed."""
    key = (shape, nb, opts)
    if key not in _REF:
        _REF[key] = _run(shape, nb, one_launch=False, opts=opts)
        dzs = [d.view(__import__("torch").float64) for d, _ in _REF[key]]
        for k in range(STEPS - 1):      # a stale value cannot hide: every entry of step k + 1 is another number
            assert bool((dzs[k + 1] != dzs[k]).all()), (shape, k)
        assert all(bool(d.isfinite().all()) for d in dzs)
    return _REF[key]


def _same(got, ref, what):
    import torch
    for k in range(STEPS):              # steps 1 and 2 are the reusing ones; step 0 (recording) runs neither path
        assert torch.equal(got[k][0], ref[k][0]), (what, k)
        assert got[k][1] == ref[k][1], (what, k, got[k][1], ref[k][1])


@pytest.mark.parametrize("shape,nb", SHAPES, ids=IDS)
def test_same_bits_as_the_per_panel_forward(shape, nb):
    _same(_run(shape, nb, one_launch=True), _ref(shape, nb), shape)


@pytest.mark.parametrize("blocks", [2, 3, 5])
@pytest.mark.parametrize("shape,nb", [SHAPES[0], SHAPES[2]], ids=[IDS[0], IDS[2]])
def test_small_grids(shape, nb, blocks):
    """2 workgroups: one owner takes every chunk; 3 and 5: the smallest strided ownerships, chunks of one panel on several owners."""
    opts = (("sweep_max_blocks", blocks),)
    ref = _ref(shape, nb, opts)
    _same(ref, _ref(shape, nb), (shape, blocks, "the per-panel forward does not depend on the grid of the sweeps"))
    _same(_run(shape, nb, one_launch=True, opts=opts), ref, (shape, blocks))


@pytest.mark.parametrize("shape,nb", [SHAPES[0], SHAPES[2]], ids=[IDS[0], IDS[2]])
def test_without_the_one_launch_sweeps_it_falls_back(shape, nb):
    """sweep_persist = 0: the per-panel loop runs (the library has no counter of k_fwd_prefix launches to show: the results say it)."""
    opts = (("sweep_persist", 0),)
    _same(_run(shape, nb, one_launch=True, opts=opts), _ref(shape, nb, opts), (shape, "sweep_persist=0"))
