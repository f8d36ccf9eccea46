"""The period that closes a segment of msk_lean.hip msk.hip's way, pinned in the product's assembly (CPU only).

One channel of a wave whose byte close cannot wait -- on idle channels the byte behind a false sync, all the time (profiles/LEDGER.md,
"Byte closes that end a segment") -- takes the whole wave through that period's framing, frame_bit() (msk_common.h).  Closes in SYN2
(SYN, ~SYN, neither), a SOH1 that is no SOH and the byte behind a block are applied there by selects, next to `hunt` and `plain`,
and decode_acars() is entered only for what is left (a sync from WSYN, a SOH, text bytes that are not plain, the CRC bytes): its
walk over the state -- pairs of s_and_saveexec / s_cbranch_execz -- has no SYN2, no END and no reset side any more.  Read off
`msk_lean_kernel<8,4,true>` (the bench's kernel) and `<8,1,true>`, compiled with the product's flags: the closing period is what
lies behind the ninth v_rsq_f64 of the kernel (eight periods of the unrolled segment and this one call decide()) up to the branch
back to the segment loop.

 (a) it holds fewer conditional branches than the parent's 26, and at most as many, and is at most as long, as in the tree that
     made the change;
 (b) with ACG_LEAN_AB_CLOSE0 (kept for same-tree A/B builds, profiles/probe/build_ab.py) it holds the parent's 26 again, i.e.
     (a) can fail.

The eight periods themselves are pinned by test_lean_issue_order.py, test_lean_chain_layout.py, test_lean_slots.py and
test_lean_record_store.py."""
import os
import shutil
from concurrent.futures import ThreadPoolExecutor

import pytest

from test_lean_slots import compile_lean

KERNELS = [(8, 4, True), (8, 1, True)]
PARENT_BRANCHES = 26
BRANCHES = 22          # the tree that made the change
LENGTH = 330           # instructions behind the ninth v_rsq_f64 (the parent: 398)
BACK = "-DACG_LEAN_AB_CLOSE0"


@pytest.fixture(scope="module")
def builds():
    if not (os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("hipcc")):
        pytest.skip("hipcc not available")
    with ThreadPoolExecutor(max_workers=2) as ex:
        got = list(ex.map(compile_lean, [[], [BACK]]))
    return dict(zip(["product", BACK], got))


def closing_period(body):
    """the instructions behind the ninth v_rsq_f64 up to and including the first unconditional branch"""
    r = [i for i, l in enumerate(body) if l.startswith("v_rsq_f64")]
    assert len(r) == 9, len(r)
    end = next(i for i in range(r[8], len(body)) if body[i].split(" ")[0] == "s_branch")
    return body[r[8] + 1:end + 1]


def branches(w):
    return sum(l.startswith("s_cbranch") for l in w)


def test_the_bound_is_below_the_parents_figure():
    assert BRANCHES < PARENT_BRANCHES


@pytest.mark.parametrize("key", KERNELS)
def test_the_closing_period_walks_fewer_states(builds, key):
    w = closing_period(builds["product"][key])
    assert branches(w) <= BRANCHES, ("<%d,%d,true>" % key[:2], branches(w), BRANCHES)
    assert len(w) <= LENGTH, ("<%d,%d,true>" % key[:2], len(w), LENGTH)
    # what is left of the state machine is still there: the block queue's counter, twice (a block that ends at DLE, the CRC2 close)
    assert sum(l.startswith("global_atomic_add") for l in w) == 2


@pytest.mark.parametrize("key", KERNELS)
def test_the_switch_back_is_the_parents_closing_period(builds, key):
    w = closing_period(builds[BACK][key])
    assert branches(w) == PARENT_BRANCHES, ("<%d,%d,true>" % key[:2], branches(w))
    assert len(w) > LENGTH
