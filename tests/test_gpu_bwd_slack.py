"""The backward sweep in one launch without chain steps for the closed-form slack panels (k_bwd_sweep).

Workgroup 0 of k_bwd_sweep leaves the panels that lie wholly inside the slack block out of its walk where the structural zeros are
skipped: x of such a panel is what v holds once the owners of its columns are through.  PYIPM_BWD_SLACK=0 (read when the handle is
created) keeps every panel on the chain.  The contributions a column receives, their order and the code that folds them are the
same either way, so every comparison is BIT FOR BIT, as int64 patterns, against a handle created with PYIPM_BWD_SLACK=0: the
direction and every statistics field of three steps of one handle (a recording and two reusing ones, then three full ones under
PYIPM_REUSE_X=0) with other s, lambda, mu and right-hand side each time, then `solve` with a right-hand side of its own and a
refined solve (refine = 2) against the last factor.

Shapes.  The library accepts panel widths that are multiples of 128 only, so no handle has nb = 64.  Each (n, me, mi) of the list
this test was asked for at nb = 64 runs twice at nb = 128: as it stands, and doubled, which gives the panel structure it has at
nb = 64 (named *_x2).  As it stands (128, 0, 192) has one whole slack panel whose right neighbour straddles n + mi = i0, so that
panel's lambda_i rows begin in the next step's panel: the case in which a left-out panel's columns receive a non-zero
contribution from the step next to them, through their ordinary owners.
All of it in the suite's NaN-filled workspace.  No test provokes a timeout: the error path is reviewed by reading."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

STEPS = 3
# name: (n, me, mi), nb
SHAPES = {
    "aligned": ((128, 64, 128), 128),
    "me0": ((128, 0, 192), 128),
    "straddles": ((100, 40, 150), 128),
    "one_x_panel": ((64, 64, 128), 128),
    "no_whole_slack_panel": ((192, 64, 32), 128),
    "aligned_x2": ((256, 128, 256), 128),               # the aligned baseline: two x panels, two slack panels
    "me0_x2": ((256, 0, 384), 128),                     # pred of the first lambda_i panel is the last x panel
    "straddles_x2": ((200, 80, 300), 128),              # both borders straddle, one whole slack panel between
    "one_x_panel_x2": ((128, 128, 256), 128),
    "no_whole_slack_panel_x2": ((384, 128, 64), 128),
    "nb256": ((512, 256, 512), 256),                    # four tiles per panel
}
BASE = "aligned_x2"
GROUP = {128: 1, 256: 2}                                # panels per group, as tests/test_gpu_slack_one_launch.py sets them
REUSING = ("aligned_x2", "me0_x2", "nb256")             # handles whose second and third step must be reusing ones


def _qp(shape):
    from pyipm_amd.problems import make_qp
    return make_qp(shape[0], shape[1], shape[2], seed=11)


def _vec(qp, k, variant=None):
    n, me, mi = qp["n"], qp["me"], qp["mi"]
    rng = np.random.default_rng(3000 + k)
    v = dict(df=qp["df"] + 0.1 * rng.standard_normal(n), ce=qp["ce"] + 0.1 * rng.standard_normal(me),
             ci=qp["ci"] + 0.1 * rng.standard_normal(mi), s=qp["s"] * rng.uniform(0.5, 2.0, mi),
             lda=qp["lam"] * rng.uniform(0.5, 2.0, me + mi), mu=0.3 / (k + 1))
    if variant == "zero_lambda":        # Sigma = 0 exactly: static pivots in the slack panels (tests/test_gpu_slack_one_launch.py)
        v["lda"][me + np.arange(5 + k, mi, 37)] = 0.0
    if variant == "flagged_tile":       # Sigma spread over 1e16 inside the tile of columns [64, 128): the refinement recurrence
        v["s"][64:128] *= 10.0 ** np.linspace(-8.0, 8.0, 64)
    return v


def _core(name, slack_walk, reuse_x, opts):
    from pyipm_amd.newton import NewtonCore
    shape, nb = SHAPES[name]
    env = {"PYIPM_BWD_SLACK": "1" if slack_walk else "0", "PYIPM_REUSE_X": "1" if reuse_x else "0"}
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
    core.set_option("group", GROUP[nb])
    for k, v in opts:                   # (before the first step: any set_option call drops a recorded prefix)
        core.set_option(k, v)
    return core


def _run(name, slack_walk, reuse_x=True, opts=(), variant=None):
    """STEPS steps of one handle, then a solve with a right-hand side of its own and a refined one: [(bits, statistics or None)]."""
    import torch
    assert os.environ.get("PYIPM_POISON_WORKSPACE")
    qp = _qp(SHAPES[name][0])
    core = _core(name, slack_walk, reuse_x, opts)
    core.stage_blocks(qp["d2L"], qp["Je"], qp["Ji"])
    out = []
    for k in range(STEPS):
        v = _vec(qp, k, variant)
        core.stage_vectors(v["df"], v["ce"], v["ci"], v["s"], v["lda"], mu=v["mu"])
        dz, st = core.step(0.0, 0.0, 0)
        info = core.reuse_info()
        if reuse_x and name in REUSING:
            assert info["reused"] == k and info["last"] == ("recording" if k == 0 else "reusing"), (name, k, info)
        elif not reuse_x:
            assert info["reused"] == 0 and info["last"] == "full", (name, k, info)
        out.append((dz.clone().view(torch.int64), dict(st, kind=info["last"])))     # (the kind of step is compared too)
    rhs = np.random.default_rng(77).standard_normal(core.N)
    out.append((core.solve(rhs, flip=False).clone().view(torch.int64), None))
    out.append((core.solve(rhs, flip=True, refine=2).clone().view(torch.int64), None))
    core.close()
    return out


_REF = {}


def _ref(name, reuse_x=True, opts=(), variant=None):
    """Every panel on the chain (PYIPM_BWD_SLACK=0) on the same inputs: computed once per key, never changed."""
    import torch
    key = (name, reuse_x, opts, variant)
    if key not in _REF:
        _REF[key] = _run(name, False, reuse_x, opts, variant)
        dzs = [d.view(torch.float64) for d, _ in _REF[key]]
        for k in range(STEPS - 1):      # a stale value cannot hide: every entry of step k + 1 is another number
            assert bool((dzs[k + 1] != dzs[k]).all()), (name, k)
        assert all(bool(d.isfinite().all()) for d in dzs)
    return _REF[key]


def _same(got, ref, what):
    import torch
    assert len(got) == len(ref) == STEPS + 2
    for k, ((g, gst), (r, rst)) in enumerate(zip(got, ref)):    # k < STEPS: steps; then the solve; then the refined solve
        assert torch.equal(g, r), (what, k, int((g != r).sum()))
        assert gst == rst, (what, k, gst, rst)


@pytest.mark.parametrize("reuse_x", [True, False], ids=["reusing", "full"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_same_bits_as_the_walk_over_every_panel(name, reuse_x):
    _same(_run(name, True, reuse_x), _ref(name, reuse_x), (name, reuse_x))


def test_without_skipped_zeros_no_panel_is_left_out():
    opts = (("skip_zeros", 0),)
    _same(_run(BASE, True, True, opts), _ref(BASE, True, opts), "skip_zeros=0")


@pytest.mark.parametrize("name", [BASE, "me0", "nb256"])
def test_one_workgroup_of_owners_holds_several_groups_a_wave_and_lags(name):
    """The smallest grid: workgroup 0, the near specialists and ONE workgroup of owners, 16 waves for 112 (BASE) column groups."""
    nearb = (SHAPES[name][1] // 8 + 15) // 16
    opts = (("sweep_max_blocks", 2 + nearb),)
    _same(_run(name, True, True, opts), _ref(name, True, opts), (name, "sweep_max_blocks"))


@pytest.mark.parametrize("reuse_x", [True, False], ids=["reusing", "full"])
def test_static_pivots_in_the_slack_panels(reuse_x):
    got, ref = _run(BASE, True, reuse_x, (), "zero_lambda"), _ref(BASE, reuse_x, (), "zero_lambda")
    assert all(st["n_zero"] > 0 for _, st in ref[:STEPS]), [st for _, st in ref[:STEPS]]
    _same(got, ref, ("zero_lambda", reuse_x))


@pytest.mark.parametrize("reuse_x", [True, False], ids=["reusing", "full"])
def test_a_flagged_slack_tile(reuse_x):
    """Sigma = lambda_i / s spreads over 1e16 inside one 64-column tile of a slack panel: the tile is flagged and refined."""
    got, ref = _run(BASE, True, reuse_x, (), "flagged_tile"), _ref(BASE, reuse_x, (), "flagged_tile")
    _same(got, ref, ("flagged_tile", reuse_x))
    assert all(st["d_max"] >= 1.0e12 * st["d_min"] for _, st in ref[:STEPS]), [st for _, st in ref[:STEPS]]
