"""The decoder of an update's status words (csrc/run_outcome.h: decode_outcome, the one table msckf_get_result,
msckf_commit_covariance and msckf_get_shared_result decide from) against DESIGN.md 3.5, "Status words", restated here in
Python: every combination of status words 0, 1, 4 in {0, 1, 2, 3}, word 1 ours or not, word 4 ours or not, K6-K7 ran or
not, 0 or 5 features accepted -- 1024 rows, printed by a driver built with the host compiler from the header alone."""
import itertools
import os
import subprocess

import pytest

from conftest import ROOT

HEADER_DIR = os.path.join(ROOT, "monocular-visual-inertial-msckf_amd", "csrc")
NAMES = ["Ok", "Noop", "NotSpd", "Timeout", "Unwritten", "Overflow"]        # enum class Outcome, in order

DRIVER = r"""
#include <cstdio>
#include "run_outcome.h"
int main() {
    for (int s0 = 0; s0 < 4; ++s0) for (int s1 = 0; s1 < 4; ++s1) for (int s4 = 0; s4 < 4; ++s4)
    for (int w1 = 0; w1 < 2; ++w1) for (int w4 = 0; w4 < 2; ++w4) for (int gain = 0; gain < 2; ++gain)
    for (int n = 0; n <= 5; n += 5) {
        const int status[5] = {s0, s1, 77, -1, s4};          // (words 2 and 3 are not the decoder's)
        std::printf("%d %d %d %d %d %d %d %d\n", s0, s1, s4, w1, w4, gain, n, (int)decode_outcome(gain, w1, w4, n, status));
    }
    return 0;
}
"""


def expected(s0, s1, s4, word1_ours, word4_ours, gain, n_accepted):
    """DESIGN.md 3.5, the table of "Status words": first match wins."""
    if n_accepted == 0:
        return "Noop"                       # 1. nothing was accepted, whatever the words say
    if not gain:
        return "Ok"                         # 2. K6-K7 did not run: no word is read
    if not word1_ours:
        s1 = 0                              # 3. a word that is not the run's reads as 0
    if not word4_ours:
        s4 = 0
    if 3 in (s0, s1):
        return "Unwritten"                  # 4. a mirror in host memory still holds its seed
    if 2 in (s0, s1):
        return "Timeout"                    # 5.
    if s0 or s1:
        return "NotSpd"                     # 6.
    if s4 & 2:
        return "Overflow"                   # 7. more remainder rows than the merge takes
    return "Ok"                             # 8.


@pytest.fixture(scope="module")
def rows(tmp_path_factory):
    d = tmp_path_factory.mktemp("run_outcome")
    src, exe = os.path.join(d, "driver.cpp"), os.path.join(d, "driver")
    with open(src, "w") as f:
        f.write(DRIVER)
    subprocess.run(["c++", "-std=c++17", "-Wall", "-Werror", "-I", HEADER_DIR, "-o", exe, src], check=True, timeout=120)
    out = subprocess.run([exe], check=True, capture_output=True, text=True, timeout=30).stdout
    return {tuple(v[:7]): NAMES[v[7]] for v in (tuple(map(int, line.split())) for line in out.splitlines())}


def test_every_row_of_the_table(rows):
    keys = list(itertools.product(range(4), range(4), range(4), (0, 1), (0, 1), (0, 1), (0, 5)))
    assert len(keys) == 1024 and set(rows) == set(keys)
    wrong = {k: (rows[k], expected(*k)) for k in keys if rows[k] != expected(*k)}
    assert not wrong, wrong


def test_rows_by_name(rows):
    # (status word 0, word 1, word 4, word 1 ours, word 4 ours, K6-K7 ran, accepted)
    for s1 in (1, 2, 3):
        assert rows[(0, s1, 0, 0, 0, 1, 5)] == "Ok"                 # word 1 non-zero but not ours
    for w1, w4, s1, s4 in itertools.product((0, 1), (0, 1), range(4), range(4)):
        assert rows[(3, s1, s4, w1, w4, 1, 5)] == "Unwritten"       # word 0 = 3
    assert rows[(1, 2, 0, 1, 0, 1, 5)] == "Timeout"                 # word 0 = 1 with word 1 = 2, ours
    assert rows[(0, 0, 2, 0, 1, 1, 5)] == "Overflow"                # bit 1 of word 4, ours, everything else clean
    assert rows[(0, 0, 2, 0, 0, 1, 5)] == "Ok"                      # ... not ours: stale
    for k, v in rows.items():
        if k[6] == 0:
            assert v == "Noop", k                                   # nothing accepted, whatever the words say
