"""The block LDL' factor that every result comes out of, entrywise against extended precision (tests/factor_check.py): one
test per distinct producer of factor entries.  Replaces the LAPACK factorisation reached from pyipm.py:18-20, 1720-1721.

Each test reads the assembled matrix K and Lb from kkt_storage() and asserts
 (a) K equals oracle.newton_oracle.kkt_matrix on the triangle bit for bit (full-form handles): the factor is chained to the
     reference;
 (b) max |R| / (eps B) <= min(MARGIN x the ratio of the NumPy model BlockLDL(K, refine = the handle's block_refine) on the same
     matrix through the same checker, Npad + 64);
 (c) the inertia read off the reconstructed block pivots, less the identity padding, equals the reported statistics (and
     Manufactured.inertia());
 (d) nonfinite == 0 and n_zero == 0;
and that the producer it is about did run, wherever the library can say so (trailing_instances(), profile option).

Which update instance a launch takes is decided in launch_update128 (csrc/pyipm_newton.hip):
  * k_update<256,true,8>: bulk_bn = 256 (default), nb % 256 == 0, col_end % 256 == 0, K >= 512, and reserve_cus <= 0 or more than
    20480 rows -- here reserve_cus = 0, nb = 256, group = 2, Npad = 1024, lookahead = 0 (with a lookahead the only bulk launch of
    a two-group system is the head, which runs as 32 x 64 blocks);
  * k_update<64,true,8>: with bulk_bn = 256 every tile-list launch of at most 5/8 of the CUs (160 of 256) tiles.  A launch over
    m rows has at most (m / 128)(m / 128 + 1) / 2 tiles, so every bulk launch of a system of at most 2176 rows takes it: the
    default-option tests below are its tests.  trailing_instances() files it under 128 (factor_end: every tag but 256), so the
    count cannot tell it from the next one; the options can;
  * k_update<128,true,8> from the tile list: bulk_bn = 128 switches both of the above off;
  * its persistent form: bulk_bn = 128, reserve_cus = CUs - 8, so that slots = 2 (CUs - reserve_cus) = 16 < the 21 tiles of the
    launch over the last 768 rows (lookahead = 0, mi = 0: no tile is structurally empty); persist_rows (12288) covers it;
  * k_update<128,false>, the plain grid of the panel-chain launches: NOT reached here.  factor_block launches it only while more
    than PENDING_LEFT_ROWS = 12288 rows lie below the group's diagonal block, factor_panel only with more than PENDING32_ROWS =
    24576 rows left; below that both use k_inpanel_update.  It stays with the large shapes of test_gpu_known_inertia.py.

Measured on an MI355X (ratio = max |R| / (eps B); growth = max B / max |K|; MARGIN = 4, the most the bound allows -- the device's
ratios sit at 1.2 .. 3.0 times the model's: MFMA sums the products in groups of four and in tile order, and the device refines
only the block solves of flagged tiles where the model refines all of them):

    case                                            Npad   device   model   bound   growth
    make_qp (203, 37, 61)                            384     3.87    2.01     8.0   5e-1
    make_qp (200, 0, 100)                            512     3.39    2.25     9.0   6e-1
    make_qp (260, 100, 0)                            384     3.48    2.04     8.2   7e-1
    make_qp (320, 128, 256)  (also lookahead 0, 2,
        skip_zeros 0: the same bits, from the cache) 1024    3.37    2.63    10.5   7e-1
    make_qp (256, 256, 1024)                        2560     4.35    2.52    10.1   2e+2     (37.32 with refine_cond = 1e3)
    graded (300, 40, 100), 7 decades  (all pivot
        kernels)                                     640     4.24    2.71    10.8   2e-1
    Manufactured(300, 60, 140, "Q", n_neg = 100)     640     6.87    5.36    21.4   8e+4
    per-panel nb = 256, graded (500, 100, 100)       896     7.10    2.35     9.4   2e-1
    per-panel nb = 1024, graded (700, 100, 200)     1280     7.23    3.76    15.0   2e-1
    graded (700, 200, 0): k_update<128,true,8> list,
        persistent, k_update<256,true,8> (same bits) 1024    6.71    2.76    11.0   2e-1
    condensed make_qp (320, 128, 256)                512     3.28    2.43     9.7   4e-1

What this module found: with refine_cond = 1e3, the default until then, make_qp (256, 256, 1024) gave 37.3 against a bound of
10.1 (model 2.52), at tile column 23 (the last tile of the lambda_e block, rows of lambda_i; me = n makes that block's Schur
complement ill-conditioned: d_min 1e-3, growth 2e2).  The model WITHOUT refinement of the block solves gives 42.1 at the same
tile column, with one step 2.44: the tile's pivot spread lay between 1e2 and 1e3, so it was not flagged and its block solve
stayed unrefined, while the spread underestimates cond(T) of a dense tile.  No update kernel was involved.  The default is 1e2
now (csrc/ctx.hpp); the device gives 4.35 there, as with refine_cond = 30 and 10 (the same bits), and 5.27 with every tile
refined.

tile_blocked = 0 does NOT give the default's bits (the blocked inversion commits 16 pivots at a time, another order of
operations; tests/test_gpu_tile_blocked.py compares the two only where no block is committed), so it gets a reconstruction of
its own; the other pivot kernels are bit-identical to the default and come out of the cache.

CPU time of one reconstruction: 0.1 s at Npad 384 .. 640, 0.4 .. 0.8 s at 1024 .. 1280, 3.0 s at 2560 (the model's reference
costs the same again, once per matrix).
"""
import numpy as np
import pytest

from factor_check import MARGIN, bound, check_factor, factor_of, model_factor
from kkt_manufactured import Manufactured
from oracle import newton_oracle as orc

pytestmark = pytest.mark.gpu

_model = {}


def _qp(n, me, mi, seed):
    from pyipm_amd.problems import make_qp
    return make_qp(n, me, mi, seed)


def _graded(n, me, mi, seed, decades):
    from test_gpu_tile_blocked import _graded_qp
    return _graded_qp(n, me, mi, seed, decades)


class _Problem(object):
    """A staged system: blocks, the oracle's matrix (computed once), the model's ratio per block_refine (computed once)."""

    def __init__(self, kind, n, me, mi, seed, decades=0.0):
        self.kind, self.n, self.me, self.mi = kind, n, me, mi
        self.key = (kind, n, me, mi, seed, decades)
        if kind == "manufactured":
            self.m = Manufactured(n, me, mi, mixer="Q", n_neg=n // 3, seed=seed)
            self.H = self.m.kkt_matrix()
        else:
            self.qp = _qp(n, me, mi, seed) if kind == "qp" else _graded(n, me, mi, seed, decades)
            q = self.qp
            self.H = orc.kkt_matrix(q["d2L"], q["Je"], q["Ji"], q["s"], q["lam"], n, me, mi)

    def stage(self, core):
        if self.kind == "manufactured":
            self.m.stage(core)
        else:
            q = self.qp
            core.stage_blocks(q["d2L"], q["Je"], q["Ji"])
            core.stage_vectors(q["df"], q["ce"], q["ci"], q["s"], q["lam"], mu=q["mu"])

    def inertia(self):
        if self.kind == "manufactured":
            neg, zero, pos = self.m.inertia()
            assert zero == 0
            return pos, neg
        return self.n + self.mi, self.me + self.mi

    def model_ratio(self, refine, A=None, neg_from=None, sigma_from=None, tag="full"):
        k = (self.key, refine, tag)
        if k not in _model:
            K, Lb, f = model_factor(self.H if A is None else A, refine=refine,
                                    neg_from=self.n + self.mi if neg_from is None else neg_from,
                                    sigma_from=self.n if sigma_from is None else sigma_from)
            assert f.stats["zero"] == 0
            _model[k] = check_factor(K, Lb)
        return _model[k]


_problems = {}


def _problem(*key):
    if key not in _problems:
        _problems[key] = _Problem(*key)
    return _problems[key]


def _handle(p, nb=128, **opts):
    from pyipm_amd.newton import NewtonCore
    core = NewtonCore(p.n, p.me, p.mi, device=0, nb=nb)
    core.set_option("expert", 1)
    core.set_option("profile", 1)
    for k, v in opts.items():
        core.set_option(k, v)
    p.stage(core)
    return core


def _per_panel(core):
    core.factor_begin()
    for q in range(core.npanels):
        core.factor_panel(q)
        core.trailing_update(q)
    return core.factor_end()


def _check(p, core, factor=None, refine=2, label=""):
    """(a) .. (d) of the module docstring for a full-form handle.  Returns (K, Lb bits, FactorCheck, stats)."""
    N, Npad = core.N, core.Npad
    K, Lb, st = factor_of(core, factor)
    assert K.shape == (Npad, Npad)
    assert np.array_equal(np.tril(K[:N, :N]), np.tril(p.H)), "assembled matrix differs from the oracle's"
    assert np.array_equal(np.tril(K[N:, N:]), np.eye(Npad - N)) and not K[N:, :N].any()
    return _judge(p, K, Lb, st, p.model_ratio(refine), Npad - N, p.inertia(), st, label)


def _judge(p, K, Lb, st, ref, pad, inertia, stats, label):
    Npad = K.shape[0]
    r = check_factor(K, Lb)
    lim = bound(ref.ratio, Npad, MARGIN)
    print("[factor] %-44s Npad %5d  device %6.2f  model %5.2f  bound %5.1f  growth %.1e  at %s  %.1f s" %
          (label or str(p.key), Npad, r.ratio, ref.ratio, lim, r.growth, r.where, r.seconds))
    assert st["nonfinite"] == 0 and st["n_zero"] == 0, st
    assert r.ratio <= lim, "ratio %.3g > %.3g (model %.3g) at (tile column, row, column) %s; growth %.2e; %s" % (
        r.ratio, lim, ref.ratio, r.where, r.growth, st)
    assert (r.n_pos - pad, r.n_neg) == inertia, (r, inertia)
    assert (stats["n_pos"], stats["n_neg"]) == inertia, (stats, inertia)
    return K, Lb, r, st


def _close(core):
    import torch
    core.close()
    torch.cuda.empty_cache()


# ---- the default single-rank schedule (nb = 128, group = 2): k_update<64,true,8>, k_inpanel_update heads, chains --------------------
DEFAULT = [("qp", 203, 37, 61, 1), ("qp", 200, 0, 100, 2), ("qp", 260, 100, 0, 3), ("qp", 320, 128, 256, 4),
           ("qp", 256, 256, 1024, 5), ("graded", 300, 40, 100, 1, 7.0), ("manufactured", 300, 60, 140, 5)]


@pytest.mark.parametrize("key", DEFAULT, ids=["-".join(str(x) for x in k) for k in DEFAULT])
def test_default_schedule(key):
    """N off the 64 grid; me = 0; mi = 0; a panel that straddles column n; slack panels in one launch (k_s_panels: eight
    closed-form panels); a graded system (flagged tiles: refined block solves); 2 x 2 pivots and growth ~1e5.  Every bulk launch
    is k_update<64,true,8> (module docstring)."""
    p = _problem(*key)
    core = _handle(p, nb=128, group=2)
    K, Lb, r, st = _check(p, core)
    inst = core.trailing_instances()
    assert inst[256]["launches"] == 0, inst
    if key[0] == "manufactured":
        assert st["n_2x2"] >= 1, st
    _close(core)


# ---- per-panel schedule -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb,key", [(256, ("graded", 500, 100, 100, 2, 4.0)), (1024, ("graded", 700, 100, 200, 3, 4.0))])
def test_per_panel_schedule(nb, key):
    """factor_begin / factor_panel / trailing_update / factor_end on one rank: nb = 256, and the wide panels of nb = 1024
    (factor_wide_panel needs columns behind the panel: Npad = 1280 > nb; the library has no counter that says it ran -- it does by
    factor_panel's condition: tile_step, no group schedule, panel_w = 1024 > wide_sub = 256, 16 tiles, columns behind it)."""
    p = _problem(*key)
    core = _handle(p, nb=nb)
    assert core.npanels >= 2
    _check(p, core, factor=_per_panel, label="per-panel nb=%d %s" % (nb, key[1:4]))
    _close(core)


# ---- update instances ---------------------------------------------------------------------------------------------------------------
INST = ("graded", 700, 200, 0, 4, 4.0)            # N = 900, Npad = 1024, mi = 0: no structurally empty tile


def test_update_128_from_the_tile_list():
    p = _problem(*INST)
    core = _handle(p, nb=128, group=2, bulk_bn=128, reserve_cus=0, lookahead=0)
    _check(p, core, label="k_update<128,true,8> tile list")
    inst = core.trailing_instances()
    assert inst[128]["launches"] >= 1 and inst[256]["launches"] == 0, inst
    _close(core)


def test_update_128_persistent():
    import torch
    p = _problem(*INST)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    core = _handle(p, nb=128, group=2, bulk_bn=128, reserve_cus=cus - 8, lookahead=0)
    # The library cannot say that the launch was persistent: trailing_instances() files it with the tile-list launch.  It is, by
    # launch_update128 (u.persist, grid.x = slots), as long as the handle's num_cus is the device's multiprocessor count --
    # which pyipm_newton_create reads from the same attribute torch reports -- so that slots = (2 * (num_cus - reserve_cus)) & ~7
    # = 16, below the 6 * 7 / 2 = 21 tiles of group 0's bulk launch over the rows [256, 1024) (mi = 0: every tile active).
    assert core.Npad == 1024
    _check(p, core, label="k_update<128,true,8> persistent")
    inst = core.trailing_instances()
    assert inst[128]["launches"] >= 1 and inst[256]["launches"] == 0, inst
    _close(core)


def test_update_256():
    p = _problem(*INST)
    core = _handle(p, nb=256, group=2, reserve_cus=0, lookahead=0)
    assert core.Npad % 256 == 0
    _check(p, core, label="k_update<256,true,8>")
    inst = core.trailing_instances()
    assert inst[256]["launches"] >= 1, inst
    _close(core)


# ---- schedule switches --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opts", [{"lookahead": 0}, {"lookahead": 2}, {"skip_zeros": 0}], ids=["lookahead0", "lookahead2", "skip_zeros0"])
def test_schedule_switches(opts):
    p = _problem("qp", 320, 128, 256, 4)
    core = _handle(p, nb=128, group=2, **opts)
    _check(p, core, label="%s %s" % (opts, p.key[1:4]))
    _close(core)


# ---- pivot kernels ------------------------------------------------------------------------------------------------------------------
def test_pivot_kernels_give_the_default_bits_and_one_reconstruction():
    """tile_chain 0 with four waves, with eight everywhere and tile_chain 2 against the default on a graded system: the same bits
    of what the factor is (Lb below the diagonal tiles), so one reconstruction serves all of them (the cache).  tile_blocked 0
    (single sweeps) rounds differently and is reconstructed by itself (module docstring)."""
    p = _problem("graded", 300, 40, 100, 1, 7.0)
    out = {}
    for name, opts in (("default", {}), ("steps4", {"tile_chain": 0, "tile_waves": 4}), ("steps8", {"tile_chain": 0, "tile_waves": 9}),
                       ("chain2", {"tile_chain": 2}), ("single_sweeps", {"tile_blocked": 0})):
        core = _handle(p, nb=128, group=2, **opts)
        K, Lb, r, st = _check(p, core, label="pivot kernels: %s" % name)
        out[name] = (K, Lb, r, st)
        _close(core)
    t = np.arange(out["default"][1].shape[0]) // 64
    below = t[:, None] > t[None, :]
    for name in ("steps4", "steps8", "chain2"):
        assert np.array_equal(out[name][1][below].view(np.int64), out["default"][1][below].view(np.int64)), name
        assert out[name][2].seconds == 0.0, (name, "not from the cache")
        assert out[name][3] == out["default"][3], (name, out[name][3], out["default"][3])
    # (the single sweeps: another order of operations than the blocked inversion, so other bits -- judged by a reconstruction
    #  of their own in _check above; the counts agree)
    keys = ("n_pos", "n_neg", "n_2x2", "n_zero", "nonfinite")
    assert [out["single_sweeps"][3][k] for k in keys] == [out["default"][3][k] for k in keys]


# ---- condensed form -----------------------------------------------------------------------------------------------------------------
def test_condensed_form():
    """set_option("condensed", 1): K is what the storage holds after assemble(), [[H + Ji Sigma Ji', Je], [Je', 0]] (plus the
    explicit rows of inequalities with a large Sigma, -1/Sigma on the diagonal), with its own ld and ncols.  The statistics are
    those of the FULL matrix: every eliminated inequality adds one positive and one negative pivot."""
    p = _problem("qp", 320, 128, 256, 4)
    core = _handle(p, nb=128, group=2, condensed=1)
    core.residual()
    K, Lb, st = factor_of(core)
    n, me, mi = p.n, p.me, p.mi
    d = np.diag(K)[n + me:]
    na = int(np.sum(d < 0))                            # inequalities kept as explicit rows
    Nc = n + me + na
    assert K.shape[0] == (Nc + 127) // 128 * 128 < core.Npad
    assert np.array_equal(np.tril(K[Nc:, Nc:]), np.eye(K.shape[0] - Nc)) and not K[Nc:, :Nc].any()
    A = np.tril(K[:Nc, :Nc]) + np.tril(K[:Nc, :Nc], -1).T
    ref = p.model_ratio(2, A=A, neg_from=n, sigma_from=n, tag="condensed")
    full = dict(st, n_pos=st["n_pos"] - mi, n_neg=st["n_neg"] - (mi - na))      # less the eliminated inequalities' pivots
    _judge(p, K, Lb, st, ref, K.shape[0] - Nc, (n, me + na), full, "condensed %s" % (p.key[1:4],))
    _close(core)
