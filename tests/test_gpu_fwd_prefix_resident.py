"""k_fwd_prefix with the owners' chunks of v kept on chip across panels and L requested one visit ahead.

Method as in test_gpu_fwd_prefix.py: three steps of one handle (a recording one, two reusing ones) with other vectors each time,
reuse_info checked, the suite's NaN-filled workspace, and every comparison BIT FOR BIT against the per-panel forward
(PYIPM_FWD_PREFIX=0) under the same options: the direction as int64 patterns and every field of the statistics.  v is compared
through the direction: a chunk that was published without being loaded, or not published at all, carries the workspace's NaN or
the values of the step before into it (every entry of step k + 1's direction is another number than step k's).

The cases are about WHERE a chunk of v lives and WHEN it goes back to global memory:
  * an owner holds FWDP_RESIDENT chunks on chip; its further ones make the global round trip on every visit.  With two workgroups
    one owner takes every chunk below panel 0: shapes with FWDP_RESIDENT, FWDP_RESIDENT + 1 and FWDP_RESIDENT + 2 of them;
  * grids of 3 and 5 workgroups: the chunks of one panel lie on several owners (the chain's wait for that panel depends on several
    publishers), and one owner holds chunks of consecutive panels (it publishes one while it carries the others); the default grid
    has a workgroup per chunk, the hole's included, so some owners own nothing;
  * with and without a slack hole (mi >= 512; mi = 0 and mi = 256): untouched chunks stay untouched.
Panel widths: a handle is only created with nb a multiple of 128 (pyipm_newton_create: nb % 128 == 0), so 64 (one tile per panel, no
in-panel step) and 192 (48 columns per wave) cannot be created; fwd_prefix_applies admits 128 and 256 and the kernel is built for
those two, both of which are here.
No test here provokes a timeout: the error path of the kernel is reviewed by reading."""
import os
import re

import pytest

from test_gpu_fwd_prefix import _ref, _run, _same

pytestmark = pytest.mark.gpu

FWDP_RESIDENT = 16          # kernels_solve.hpp: the chunks of v an owner keeps on chip; the shapes below are chosen for this value


def _chunks_below_panel0(shape, nb):
    """The 64-row chunks that the owners share: those below panel 0 without the slack hole (k_fwd_prefix's nlog)."""
    n, me, mi = shape
    npad = (n + me + 2 * mi + 127) // 128 * 128
    hole = 0
    if mi >= 512:
        a, b = (n + 192 + 63) // 64, (n + mi - 256) // 64 + 1
        hole = max(b - a, 0)
    return npad // 64 - nb // 64 - hole


# one owner (two workgroups) with FWDP_RESIDENT, + 1 and + 2 chunks: all resident; one and two on the global round trip
CAPACITY = [((512, 128, 256), 128, FWDP_RESIDENT), ((256, 0, 576), 128, FWDP_RESIDENT + 1), ((512, 256, 256), 128, FWDP_RESIDENT + 2)]


def test_the_capacity_stated_here_is_the_kernels():
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "pyipm_amd", "csrc", "kernels_solve.hpp")).read()
    m = re.search(r"constexpr int FWDP_RESIDENT = (\d+);", src)
    assert m and int(m.group(1)) == FWDP_RESIDENT
    for shape, nb, want in CAPACITY:
        assert _chunks_below_panel0(shape, nb) == want, (shape, nb)


@pytest.mark.parametrize("shape,nb,chunks", CAPACITY, ids=["at_capacity", "one_over", "two_over"])
def test_one_owner_at_and_beyond_the_resident_capacity(shape, nb, chunks):
    opts = (("sweep_max_blocks", 2),)
    _same(_run(shape, nb, one_launch=True, opts=opts), _ref(shape, nb, opts), (shape, chunks))


@pytest.mark.parametrize("blocks", [3, 5, 0])
@pytest.mark.parametrize("shape,nb", [((512, 128, 256), 128), ((1024, 256, 512), 256)], ids=["n512", "n1024_nb256"])
def test_chunks_of_a_panel_on_several_owners_and_owners_over_several_panels(shape, nb, blocks):
    """3 and 5 workgroups: 2 and 4 owners, strided over panels of 2 and 4 chunks.  0: the default grid, one workgroup per chunk
    below panel 0 counted WITH the hole's chunks -- at (1024, 256, 512) two owners own nothing."""
    opts = (("sweep_max_blocks", blocks),) if blocks else ()
    _same(_run(shape, nb, one_launch=True, opts=opts), _ref(shape, nb, opts), (shape, blocks))


@pytest.mark.parametrize("shape,nb", [((1024, 256, 512), 256), ((256, 0, 576), 128), ((512, 128, 0), 128), ((512, 128, 256), 128)],
                         ids=["hole_nb256", "hole_nb128", "mi0", "mi256"])
@pytest.mark.parametrize("blocks", [2, 4])
def test_with_and_without_a_slack_hole(shape, nb, blocks):
    opts = (("sweep_max_blocks", blocks),)
    _same(_run(shape, nb, one_launch=True, opts=opts), _ref(shape, nb, opts), (shape, blocks))
