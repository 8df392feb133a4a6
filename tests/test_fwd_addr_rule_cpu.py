"""CPU: which form the forward's gathers take (``sngnn_amd/csrc/fwd_plan.h``: ``fwd_buffer_form``) as a host compiler
computes it - buffer resources iff the table has fewer than 2^31 bytes (an offset with bit 31 set must lie beyond every
array a resource names; the graph's own arrays are held to the same limit), the flat form always under
``sngnn_tuning_set(11, 1)``.  No 2 GiB table is allocated anywhere: the rule is plain C++ on byte counts."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include <stdio.h>
#include "fwd_plan.h"
int main()
{
    long long t, x, m;
    while (scanf("%lld %lld %lld", &t, &x, &m) == 3) printf("%d\n", sngnn::fwd_buffer_form(t, x, (int)m) ? 1 : 0);
    return 0;
}
"""

LIMIT = 1 << 31
# ogbn-products: 2 449 029 nodes, 61 859 140 directed edges (+ a loop per node), 100 channels
PRODUCTS_TABLE = 2449029 * 100 * 4
PRODUCTS_INDEX = max(4 * (61859140 * 2 + 2449029), 16 * 2449029)
ARXIV_TABLE, ARXIV_INDEX = 169343 * 40 * 4, 4 * (1166243 + 169343)

# (table bytes, index bytes, knob 11) -> buffer form?
CASES = [
    ((LIMIT - 1, ARXIV_INDEX, 0), True),
    ((LIMIT, ARXIV_INDEX, 0), False),
    ((LIMIT + 1, ARXIV_INDEX, 0), False),
    ((PRODUCTS_TABLE, PRODUCTS_INDEX, 0), True),
    ((ARXIV_TABLE, ARXIV_INDEX, 0), True),
    ((0, 0, 0), True),
    ((4 * LIMIT, ARXIV_INDEX, 0), False),               # a table whose size does not fit 32 bits at all
    # the knob: flat always
    ((LIMIT - 1, ARXIV_INDEX, 1), False),
    ((PRODUCTS_TABLE, PRODUCTS_INDEX, 1), False),
    ((ARXIV_TABLE, ARXIV_INDEX, 1), False),
    # the graph's own arrays under the same limit
    ((ARXIV_TABLE, LIMIT - 1, 0), True),
    ((ARXIV_TABLE, LIMIT, 0), False),
]


def test_buffer_form_iff_the_table_is_below_two_gib(tmp_path):
    assert PRODUCTS_TABLE < LIMIT and PRODUCTS_INDEX < LIMIT
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    src, exe = tmp_path / "rule.cpp", tmp_path / "rule"
    src.write_text(PROGRAM)
    subprocess.check_call([cxx, "-std=c++17", "-O0", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "sngnn_amd", "csrc"), str(src), "-o", str(exe)])
    text = "".join("%d %d %d\n" % c for c, _ in CASES)
    out = subprocess.run([str(exe)], input=text.encode(), capture_output=True, check=True).stdout.split()
    got = [int(v) == 1 for v in out]
    assert got == [want for _, want in CASES], list(zip(CASES, got))
