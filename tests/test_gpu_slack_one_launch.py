"""The closed-form slack panels of a group schedule in one launch (k_s_panels).

enqueue_slack_first queues the panels that lie inside the slack block up front.  PYIPM_SLACK_ONE=0 (read when the handle is
created) gives every one of them its own k_s_panel launch with an event behind it; otherwise one k_s_panels launch per contiguous
run of them does, a workgroup per panel, and their forward substitution waits for the one event behind it.  Every workgroup does
what one k_s_panel launch does and the statistics are atomic integer sums, minima and maxima, so every comparison is BIT FOR BIT:
the direction as int64 patterns, every statistics field, and -- after the last step -- the slack columns of the storage from the
diagonal down (L in their lambda_i rows included).  Three steps of one handle with other s, lambda, mu and right-hand side each
time: a recording one and two reusing ones, then again under PYIPM_REUSE_X=0 (three full steps); reuse_info() says which ran.
All of it in the suite's NaN-filled workspace."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

STEPS = 3
# name: (n, me, mi), nb, group
SHAPES = {
    "two_panels": ((256, 256, 256), 128, 1),
    "straddles_borders": ((256, 256, 192), 128, 1),     # Npad = 896: slack columns outside every fast panel
    "me0": ((256, 0, 256), 128, 1),
    "one_panel": ((256, 256, 128), 128, 1),
    "nb256": ((1024, 512, 512), 256, 2),                # four-tile panels: every wave of a workgroup has a tile
    "eight_panels": ((256, 256, 1024), 128, 1),         # more workgroups than tiles per panel
}
FIRST = "two_panels"


def _qp(shape):
    from pyipm_amd.problems import make_qp
    return make_qp(shape[0], shape[1], shape[2], seed=11)


def _vec(qp, k, variant=None):
    n, me, mi = qp["n"], qp["me"], qp["mi"]
    rng = np.random.default_rng(3000 + k)
    v = dict(df=qp["df"] + 0.1 * rng.standard_normal(n), ce=qp["ce"] + 0.1 * rng.standard_normal(me),
             ci=qp["ci"] + 0.1 * rng.standard_normal(mi), s=qp["s"] * rng.uniform(0.5, 2.0, mi),
             lda=qp["lam"] * rng.uniform(0.5, 2.0, me + mi), mu=0.3 / (k + 1))
    if variant == "zero_lambda":        # Sigma = 0 exactly: static pivots, in both panels, other columns at every step
        v["lda"][me + np.arange(5 + k, mi, 37)] = 0.0
    if variant == "flagged_tile":       # Sigma spread over 1e16 inside the tile of columns [64, 128): the refinement recurrence
        v["s"][64:128] *= 10.0 ** np.linspace(-8.0, 8.0, 64)
    return v


def _core(name, one_launch, reuse_x):
    from pyipm_amd.newton import NewtonCore
    shape, nb, group = SHAPES[name]
    env = {"PYIPM_SLACK_ONE": "1" if one_launch else "0", "PYIPM_REUSE_X": "1" if reuse_x else "0"}
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)                                      # (read when the handle is created)
    try:
        core = NewtonCore(shape[0], shape[1], shape[2], device=0, nb=nb)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k)
            else:
                os.environ[k] = v
    core.set_option("expert", 1)
    core.set_option("group", group)
    return core


def _run(name, one_launch, reuse_x=True, variant=None):
    """STEPS steps of one handle: [(dz bits, statistics)] and the bits of the slack columns of the storage behind the last one."""
    import torch
    assert os.environ.get("PYIPM_POISON_WORKSPACE")
    (n, me, mi) = SHAPES[name][0]
    qp = _qp(SHAPES[name][0])
    core = _core(name, one_launch, reuse_x)
    core.stage_blocks(qp["d2L"], qp["Je"], qp["Ji"])
    out = []
    for k in range(STEPS):
        v = _vec(qp, k, variant)
        core.stage_vectors(v["df"], v["ce"], v["ci"], v["s"], v["lda"], mu=v["mu"])
        dz, st = core.step(0.0, 0.0, 0)
        info = core.reuse_info()
        if reuse_x:
            assert info["reused"] == k and info["last"] == ("recording" if k == 0 else "reusing"), (name, k, info)
        else:
            assert info["reused"] == 0 and info["last"] == "full", (name, k, info)
        out.append((dz.clone().view(torch.int64), st))
    cols = core.kkt_storage()[n:n + mi, n:]                     # row j: slack column n + j from row n on
    lower = torch.arange(cols.shape[1], device=cols.device)[None, :] >= torch.arange(mi, device=cols.device)[:, None]
    slack = cols.clone().view(torch.int64)[lower].cpu()
    core.close()
    return out, slack


_REF = {}


def _ref(name, reuse_x=True, variant=None):
    """The per-panel launches (PYIPM_SLACK_ONE=0) on the same inputs: computed once per key, never changed."""
    import torch
    key = (name, reuse_x, variant)
    if key not in _REF:
        _REF[key] = _run(name, False, reuse_x, variant)
        dzs = [d.view(torch.float64) for d, _ in _REF[key][0]]
        for k in range(STEPS - 1):      # a stale value cannot hide: every entry of step k + 1 is another number
            assert bool((dzs[k + 1] != dzs[k]).all()), (name, k)
        assert all(bool(d.isfinite().all()) for d in dzs)
    return _REF[key]


def _same(got, ref, what):
    import torch
    for k in range(STEPS):
        assert torch.equal(got[0][k][0], ref[0][k][0]), (what, k)
        assert got[0][k][1] == ref[0][k][1], (what, k, got[0][k][1], ref[0][k][1])
    assert torch.equal(got[1], ref[1]), (what, "slack columns of the storage")


@pytest.mark.parametrize("reuse_x", [True, False], ids=["reusing", "full"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_same_bits_as_the_per_panel_launches(name, reuse_x):
    _same(_run(name, True, reuse_x), _ref(name, reuse_x), (name, reuse_x))


@pytest.mark.parametrize("reuse_x", [True, False], ids=["reusing", "full"])
def test_static_pivots_in_the_slack_panels(reuse_x):
    got, ref = _run(FIRST, True, reuse_x, "zero_lambda"), _ref(FIRST, reuse_x, "zero_lambda")
    assert all(st["n_zero"] > 0 for _, st in ref[0]), [st for _, st in ref[0]]
    _same(got, ref, ("zero_lambda", reuse_x))


@pytest.mark.parametrize("reuse_x", [True, False], ids=["reusing", "full"])
def test_a_flagged_tile_takes_the_refinement_recurrence(reuse_x):
    """Sigma = lambda_i / s spreads over 1e16 inside one 64-column tile, far beyond refine_cond = 1e2: the tile is flagged and L of its
    columns goes through the refinement recurrence (block_refine = 2 steps)."""
    got, ref = _run(FIRST, True, reuse_x, "flagged_tile"), _ref(FIRST, reuse_x, "flagged_tile")
    _same(got, ref, ("flagged_tile", reuse_x))
    assert all(st["d_max"] >= 1.0e12 * st["d_min"] for _, st in ref[0]), [st for _, st in ref[0]]
