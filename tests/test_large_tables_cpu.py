"""The blocks construction of tests/large_tables.py: the placement arithmetic of every case the GPU tests use, and
its premise - a block's results do not depend on where the block sits - on the oracle at a small node count."""
import pytest
import torch

from oracle.sngnn_oracle import aggregate_reference
from tests import large_tables as LT
from tests.large_tables import P


@pytest.mark.parametrize("name", sorted(LT.CASES))
def test_placement(name):
    row_size, boundaries, ntot = LT.CASES[name]
    pl = LT.place(row_size, boundaries, ntot)
    LT.check_placement(pl, row_size, boundaries)
    if ntot is None:
        # the smallest ntot that fits the blocks: the block of the largest boundary is the last one, and a table one
        # block shorter does not hold that boundary's row strictly inside a block any more
        assert pl.ntot == max(pl.offsets) + P and max(pl.offsets) < pl.boundary_rows[-1] < pl.ntot - 1
    else:
        assert pl.ntot == ntot
    LT.check_placement(LT.control(pl), row_size)


def test_the_cases_sit_where_the_issue_puts_them():
    assert LT.place(*LT.CASES["c512_last_buffer"]).ntot == 1048575 and 1048575 * 2048 == 2 ** 31 - 2048
    assert LT.place(*LT.CASES["c512_first_flat"]).ntot == 1048576
    big = LT.place(*LT.CASES["c512_past_4gib"])
    assert 2097152 < big.ntot <= 2097152 + P and big.ntot * 2048 > 2 ** 32 and len(big.offsets) == 3
    assert 13421772 * 160 < 2 ** 31 <= 13421773 * 160
    assert LT.place(*LT.CASES["c512_bf16"]).ntot == big.ntot and big.ntot * 1024 > 2 ** 31
    below, at = LT.place(*LT.CASES["lin_below"]).ntot, LT.place(*LT.CASES["lin_at"]).ntot
    assert at * 512 == LT.LIN_LIM and below == at - 16
    assert LT.place(*LT.CASES["lin_past_4gib"]).ntot * 512 > 2 ** 32
    n = LT.place(*LT.CASES["linnorm_last"]).ntot
    assert n * 160 < LT.LIN_LIM <= (n + 1) * 160 and n % 16 != 0


def test_boundary_offset_off_the_period():
    """A boundary row that is the first or the last row of a period gets a block of its own around it."""
    for r in (5 * P, 5 * P + P - 1):
        t, row = LT.boundary_offset(8, 8 * r)
        assert row == r and t < r < t + P - 1 and t % P != 0
    t, row = LT.boundary_offset(8, 8 * (5 * P + 1))
    assert (t, row) == (5 * P, 5 * P + 1)


@pytest.mark.parametrize("loops", [(False, False), (True, False), (True, True)], ids=["none", "add", "add_remove"])
@pytest.mark.parametrize("k,thr", [(16, 0.0), (4, 0.9), (None, 0.0)])
def test_premise_on_the_oracle(k, thr, loops):
    """Blocks at small offsets - one on the period, one off it, one that ends the table - give the oracle the same
    ``out`` rows and, less the offset, the same selection as the near block and as the block alone."""
    C = 8
    ei, hb = LT.edges(), LT.rows(C)
    pl = LT.Placement(5 * P + 7, (0, 2 * P, 4 * P + 7), ())
    LT.check_placement(pl, 4 * C)
    h = LT.periodic(hb, pl.ntot, pl.offsets)
    assert torch.equal(h[4 * P + 7:], hb) and torch.equal(h[P:2 * P], hb)
    kw = dict(add_loops=loops[0], remove_loops=loops[1], top_k=k, thr=thr)
    alone = aggregate_reference(hb, ei, **kw)
    big = aggregate_reference(h, LT.block_edges(ei, pl.offsets), **kw)
    assert bool((alone["out"] != 0).any())
    for t in pl.offsets:
        assert torch.equal(big["out"][t:t + P], alone["out"]), f"out of the block at {t}"
        if k is not None:
            sel = big["sel_src"][t:t + P]
            assert torch.equal(torch.where(sel >= 0, sel - t, sel), alone["sel_src"]), f"selection of the block at {t}"
    # nothing but the blocks (and the loops the mode adds): the rows in between aggregate at most themselves
    between = torch.ones(pl.ntot, dtype=torch.bool)
    for t in pl.offsets:
        between[t:t + P] = False
    tgt = big["ei"][1]
    assert bool((big["ei"][0][between[tgt]] == tgt[between[tgt]]).all())
