"""Reuse of the x-block factorisation while the staged blocks stay (pyipm_newton_reuse_info).

The x-block panels depend on the staged blocks and delta alone, so pyipm_newton_step factors them once per stage_blocks: the
first step records, the later ones reuse.  Every step here is compared BIT FOR BIT -- direction, every field of the statistics,
the KKT storage after the step -- with one step of a fresh handle that has the feature switched off (PYIPM_REUSE_X=0: the
plain full factorisation), and a test only counts where the reuse counter says that the step it means did reuse.  nb = 128 and
the expert option group = 2: systems of a few hundred rows then have several groups inside the x block.  (Reading the storage
hands its pointer out, after which a handle runs full steps only: the storage is compared after the LAST step of a sequence,
and sequences of every length are run where every step's storage matters.)"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPE = (512, 128, 256)          # N = 1152: two prefix groups, a slack group, multiplier groups


def _qp(shape, seed=3):
    from pyipm_amd.problems import make_qp
    return make_qp(shape[0], shape[1], shape[2], seed=seed)


def _vec(qp, k):
    """Vectors of step k: other s, lda, mu and right-hand side each time."""
    n, me, mi = qp["n"], qp["me"], qp["mi"]
    rng = np.random.default_rng(1000 + k)
    return dict(df=qp["df"] + 0.1 * rng.standard_normal(n), ce=qp["ce"] + 0.1 * rng.standard_normal(me),
                ci=qp["ci"] + 0.1 * rng.standard_normal(mi), s=qp["s"] * rng.uniform(0.5, 2.0, mi),
                lda=qp["lam"] * rng.uniform(0.5, 2.0, me + mi), mu=0.2 / (k + 1))


def _core(shape, group=2, reuse=True, opts=()):
    from pyipm_amd.newton import NewtonCore
    saved = os.environ.get("PYIPM_REUSE_X")
    os.environ["PYIPM_REUSE_X"] = "1" if reuse else "0"          # (read when the handle is created)
    try:
        core = NewtonCore(shape[0], shape[1], shape[2], device=0, nb=128)
    finally:
        if saved is None:
            os.environ.pop("PYIPM_REUSE_X")
        else:
            os.environ["PYIPM_REUSE_X"] = saved
    core.set_option("expert", 1)
    core.set_option("group", group)
    for k, v in opts:
        core.set_option(k, v)
    return core


def _stage(core, blocks):
    core.stage_blocks(blocks["d2L"], blocks["Je"], blocks["Ji"])


def _step(core, v, delta=0.0, delta_c=0.0, refine=0):
    core.stage_vectors(v["df"], v["ce"], v["ci"], v["s"], v["lda"], mu=v["mu"])
    return core.step(delta, delta_c, refine)


def _bits(core):
    import torch
    return core.kkt_storage().clone().view(torch.int64)


_REF = {}


def _fresh(shape, blocks, v, key, delta=0.0, delta_c=0.0, refine=0, group=2, opts=()):
    """One step of a fresh handle without the feature: (dz, stats, storage bits).  Computed once per key."""
    if key not in _REF:
        core = _core(shape, group, reuse=False, opts=opts)
        _stage(core, blocks)
        dz, st = _step(core, v, delta, delta_c, refine)
        assert core.reuse_info() == {"reused": 0, "recorded": 0, "snapshot_bytes": 0, "last": "full"}
        _REF[key] = (dz.clone(), st, _bits(core))
        core.close()
    return _REF[key]


def _same(got, ref, what, storage_of=None):
    import torch
    dz, st = got
    assert torch.equal(dz.view(torch.int64), ref[0].view(torch.int64)), what
    assert st == ref[1], (what, st, ref[1])
    if storage_of is not None:
        assert torch.equal(_bits(storage_of), ref[2]), what


def test_three_steps_equal_fresh_handles():
    qp = _qp(SHAPE)
    for last in (1, 2, 3):                                     # the storage after step 1, 2 and 3
        core = _core(SHAPE)
        _stage(core, qp)
        for k in range(last):
            got = _step(core, _vec(qp, k))
            info = core.reuse_info()
            assert info["last"] == ("recording" if k == 0 else "reusing") and info["reused"] == k and info["recorded"] == 1
            assert info["snapshot_bytes"] > 0
            _same(got, _fresh(SHAPE, qp, _vec(qp, k), ("three", k)), (last, k), core if k + 1 == last else None)
        t = core.timings()
        assert all(np.isfinite(x) for x in t.values() if isinstance(x, float))
        core.close()


def test_restaged_blocks_are_factored_again():
    qp, qp2 = _qp(SHAPE), _qp(SHAPE, seed=8)
    core = _core(SHAPE)
    _stage(core, qp)
    _step(core, _vec(qp, 0)); _step(core, _vec(qp, 1))
    assert core.reuse_info()["reused"] == 1
    _stage(core, qp2)
    got = _step(core, _vec(qp2, 2))
    assert core.reuse_info()["reused"] == 1 and core.reuse_info()["last"] == "recording"
    _same(got, _fresh(SHAPE, qp2, _vec(qp2, 2), "restaged"), "restaged", core)
    core.close()


@pytest.mark.parametrize("shift", [(1e-3, 0.0), (0.0, 1e-6)], ids=["delta", "delta_c"])
def test_another_shift_runs_in_full(shift):
    """A step with other shifts runs in full and records nothing (a shift loop changes them every call); the same shifts a
    second time in a row record, a third time reuse."""
    qp = _qp(SHAPE)
    core = _core(SHAPE)
    _stage(core, qp)
    _step(core, _vec(qp, 0)); _step(core, _vec(qp, 1))
    assert core.reuse_info()["reused"] == 1
    for k, kind in ((2, "full"), (3, "recording"), (4, "reusing")):
        got = _step(core, _vec(qp, k), *shift)
        assert core.reuse_info()["last"] == kind and core.reuse_info()["reused"] == (2 if k == 4 else 1)
        _same(got, _fresh(SHAPE, qp, _vec(qp, k), ("shift", shift, k), *shift), (shift, k), core if k == 4 else None)
    core.close()


def test_set_option_drops_the_prefix():
    qp = _qp(SHAPE)
    core = _core(SHAPE)
    _stage(core, qp)
    _step(core, _vec(qp, 0)); _step(core, _vec(qp, 1))
    assert core.reuse_info()["reused"] == 1
    core.set_option("pivtol_rel", 1e-14)                       # (its default: any set_option call drops it)
    got = _step(core, _vec(qp, 2))
    assert core.reuse_info()["reused"] == 1 and core.reuse_info()["last"] == "recording"
    _same(got, _fresh(SHAPE, qp, _vec(qp, 2), ("three", 2)), "set_option", core)
    core.close()


def _phases(core, v, refine=0):
    core.stage_vectors(v["df"], v["ce"], v["ci"], v["s"], v["lda"], mu=v["mu"])
    core.residual(); core.assemble(0.0, 0.0)
    st = core.factor()
    return core.solve(flip=True, refine=refine), st


def test_separate_phases_give_the_bits_they_always_gave():
    """assemble / factor / solve as separate calls (the QP loop of pyipm_amd/ipm.py): the same direction, statistics and
    factor as on a handle without the feature, whether the pair records, reuses or follows a fused step; the matrix a caller
    reads between assemble and factor is the whole matrix, and reading it ends the reuse."""
    import torch
    qp = _qp(SHAPE)
    ref = _core(SHAPE, reuse=False)
    _stage(ref, qp)
    core = _core(SHAPE)
    _stage(core, qp)
    for k, kind in ((0, "recording"), (1, "reusing"), (2, "reusing")):
        dz_ref, st_ref = _phases(ref, _vec(qp, k))
        dz, st = _phases(core, _vec(qp, k))
        assert core.reuse_info()["last"] == kind, (k, core.reuse_info())
        assert st == st_ref and torch.equal(dz.view(torch.int64), dz_ref.view(torch.int64)), k
    got = _step(core, _vec(qp, 3))                               # a fused step behind them reuses what they kept
    assert core.reuse_info()["reused"] == 3
    _same(got, _fresh(SHAPE, qp, _vec(qp, 3), ("three", 3)), "fused after phases")
    v = _vec(qp, 4)
    for c in (ref, core):
        c.stage_vectors(v["df"], v["ce"], v["ci"], v["s"], v["lda"], mu=v["mu"])
        c.residual(); c.assemble(0.0, 0.0)
    assert torch.equal(_bits(core), _bits(ref))                  # between the phases: the whole matrix, as ever
    st_ref, st = ref.factor(), core.factor()
    assert core.reuse_info()["last"] == "full" and core.reuse_info()["reused"] == 3
    assert st == st_ref and torch.equal(_bits(core), _bits(ref))
    assert torch.equal(core.solve().view(torch.int64), ref.solve().view(torch.int64))
    ref.close(); core.close()


def test_switched_off_never_reuses():
    qp = _qp(SHAPE)
    core = _core(SHAPE, reuse=False)
    _stage(core, qp)
    for k in range(3):
        got = _step(core, _vec(qp, k))
        _same(got, _fresh(SHAPE, qp, _vec(qp, k), ("three", k)), k)
    assert core.reuse_info() == {"reused": 0, "recorded": 0, "snapshot_bytes": 0, "last": "full"}
    core.close()


@pytest.mark.parametrize("shape,group,applies", [
    ((384, 128, 256), 2, True),        # a group straddles column n
    ((320, 128, 256), 2, True),        # a panel straddles it
    ((512, 0, 256), 2, True),          # me = 0
    ((512, 128, 0), 2, True),          # mi = 0: no slack block, the multiplier block right behind the prefix
    ((128, 128, 256), 2, False),       # the first group reaches beyond the x block: off
    ((384, 128, 192), 2, True),        # N = 896 = 7 x 128 rows, in the suite's NaN-filled workspace: three steps
], ids=["group_straddles_n", "panel_straddles_n", "me0", "mi0", "no_prefix", "odd_multiple_of_128"])
def test_boundary_shapes(shape, group, applies):
    assert os.environ.get("PYIPM_POISON_WORKSPACE")
    qp = _qp(shape, seed=5)
    for last in (2, 3):
        core = _core(shape, group)
        _stage(core, qp)
        for k in range(last):
            got = _step(core, _vec(qp, k))
            assert core.reuse_info()["reused"] == (k if applies else 0), (shape, k, core.reuse_info())
            assert np.isfinite(got[0].cpu().numpy()).all()
            _same(got, _fresh(shape, qp, _vec(qp, k), ("shape", shape, k), group=group), (shape, k), core if k + 1 == last else None)
        core.close()


@pytest.mark.parametrize("name", ["lp", "zerodiag", "linear_vars"])
def test_pivot_state_of_the_prefix_is_kept(name):
    """Tiles of the prefix take static pivots (lp: every x pivot; linear_vars) or 2 x 2 pivots (zerodiag): the blocks of
    tests/golden/pivot_*.npz, built as tests/test_gpu_pivoting.py builds them.  The sweeps of a reusing step read the kept tile
    inverses, flags and perturbed pivots; the adaptive refinement turns them into the unperturbed system's solution."""
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pivot_%s.npz" % name))
    n, me, mi = int(d["nvar"]), int(d["neq"]), int(d["nineq"])
    x, Q, A, G = d["x"], d["Q"], d["A"], d["G"]
    blocks = dict(d2L=Q, Je=np.ascontiguousarray(A.T) if me else None, Ji=np.ascontiguousarray(G.T) if mi else None)
    base = dict(n=n, me=me, mi=mi, df=Q @ x + d["c"], ce=(A @ x - d["b"]) if me else np.zeros(0), ci=G @ x - d["h"],
                s=d["s"], lam=d["lda"])
    shape = (n, me, mi)
    core = _core(shape, group=1)
    _stage(core, blocks)
    seen = None
    for k in range(3):
        got = _step(core, _vec(base, k), refine=-1)
        assert core.reuse_info()["reused"] == k
        ref = _fresh(shape, blocks, _vec(base, k), ("pivot", name, k), refine=-1, group=1)
        _same(got, ref, (name, k), core if k == 2 else None)
        seen = got[1]
    assert seen["n_zero"] > 0 or seen["n_2x2"] > 0, seen            # the fixture does what it is here for
    core.close()


@pytest.mark.parametrize("refine", [2, -1])
def test_refinement_on_a_reusing_step(refine):
    qp = _qp(SHAPE)
    core = _core(SHAPE)
    _stage(core, qp)
    _step(core, _vec(qp, 0))
    got = _step(core, _vec(qp, 1), refine=refine)
    assert core.reuse_info()["last"] == "reusing"
    _same(got, _fresh(SHAPE, qp, _vec(qp, 1), ("refine", refine), refine=refine), refine, core)
    core.close()


def test_recording_policy():
    """A caller that restages before every step (an NLP loop) pays for ONE snapshot; two steps on the same blocks start the
    recording again."""
    qp = _qp(SHAPE)
    core = _core(SHAPE)
    for k in range(4):
        _stage(core, qp)
        got = _step(core, _vec(qp, k))
        assert core.reuse_info()["recorded"] == 1 and core.reuse_info()["reused"] == 0
        assert core.reuse_info()["last"] == ("recording" if k == 0 else "full")
        if k == 3:
            _same(got, _fresh(SHAPE, qp, _vec(qp, 3), ("three", 3)), "full step of a handle that stopped recording")
    _step(core, _vec(qp, 1))                                     # the second step on the same blocks records ...
    assert core.reuse_info()["recorded"] == 2 and core.reuse_info()["last"] == "recording"
    got = _step(core, _vec(qp, 2))                               # ... and the third reuses
    assert core.reuse_info()["reused"] == 1
    _same(got, _fresh(SHAPE, qp, _vec(qp, 2), ("three", 2)), "policy", core)
    core.close()
