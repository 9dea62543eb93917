"""Every stage on a used handle against the bits of a fresh handle (tests/handle_history.py).

The kernels are deterministic -- fixed-order sums, no floating-point atomics, counter-based samples --, so "what a handle
did before does not change what a call returns now" needs no tolerance: every output of every catalogue entry after every
past, and of every solver entry at every step of the problem sequences, is the bytes a handle that did nothing else
returns.  The control `test_two_fresh_handles_agree` holds the same for two fresh handles; no output needed a bound."""
import pytest

import handle_history as hh

pytestmark = pytest.mark.gpu

_fresh = {}            # entry -> outputs of a handle that did nothing else


def new_backend():
    import sfmba
    return sfmba.Backend(0)


def fresh_outputs(name):
    """The entry on a handle of its own, computed once per module."""
    if name not in _fresh:
        be = new_backend()
        try:
            _fresh[name] = hh.ENTRIES[name]["fn"](be, hh.inputs("entry"))
        finally:
            be.close()
        assert len(_fresh[name]) > 0, f"{name}: no output to compare"
    return _fresh[name]


def assert_same(got, want, what):
    assert len(want) > 0, f"{what}: no output to compare"
    bad = hh.differing(got, want)
    assert not bad, f"{what}: {bad} differ from the fresh handle ({len(want)} outputs compared)"


@pytest.mark.parametrize("name", list(hh.ENTRIES))
def test_two_fresh_handles_agree(name):
    """The control on the reference side: a second handle that did nothing else returns the same bytes."""
    want = fresh_outputs(name)
    be = new_backend()
    try:
        got = hh.ENTRIES[name]["fn"](be, hh.inputs("entry"))
    finally:
        be.close()
    assert_same(got, want, f"{name} on a second fresh handle")


def test_every_pair_is_generated():
    n = len(hh.PAIRS)
    print(f"{len(hh.ENTRIES)} entries x {len(hh.PASTS)} pasts - {len(hh.EXCLUDED)} excluded = {n} pairs")
    for pair, reason in sorted(hh.EXCLUDED.items()):
        print(f"  excluded {pair}: {reason}")
    assert n == len(hh.ENTRIES) * len(hh.PASTS) - len(hh.EXCLUDED) and len(set(hh.PAIRS)) == n
    # the counts themselves: an entry, a past or a family member that goes missing shows here
    assert (len(hh.ENTRIES), len(hh.PASTS), len(hh.EXCLUDED), n) == (34, 7, 30, 208)
    assert all(e in hh.ENTRIES and p in hh.PASTS and reason for (e, p), reason in hh.EXCLUDED.items())


@pytest.mark.parametrize("name,past", hh.PAIRS, ids=[f"{e}-after-{p}" for e, p in hh.PAIRS])
def test_entry_after_a_past_equals_the_fresh_handle(name, past):
    want = fresh_outputs(name)
    be = new_backend()
    try:
        hh.PASTS[past](be, name)
        got = hh.ENTRIES[name]["fn"](be, hh.inputs("entry"))
    finally:
        be.close()
    assert_same(got, want, f"{name} after the past '{past}'")


@pytest.mark.parametrize("name", hh.SEQUENCES)
def test_problem_sequence_equals_fresh_handles_at_every_step(name):
    """One handle walks the sequence; at every step every solver entry equals a fresh handle given that step alone, and
    the re-use of the previous problem is what the host's table build defines."""
    walk = new_backend()
    try:
        for k, s in enumerate(hh.sequence(name)):
            what = f"{name}[{k}] ({s['note']})"
            assert hh.apply_step(walk, s) == s["ok"], what
            if not s["ok"]:
                continue
            if s["reuse"] is not None:
                assert walk.problem_reuse()[0] == s["reuse"], (what, walk.problem_reuse(), s["reuse"])
            alone = new_backend()
            try:
                assert hh.apply_step(alone, s) and alone.problem_reuse()[0] == 0, what
                want = hh.step_outputs(alone, s)
            finally:
                alone.close()
            got = hh.step_outputs(walk, s)
            assert set(got) == set(want)
            for entry in want:
                assert_same(got[entry], want[entry], f"{what}: {entry}")
    finally:
        walk.close()


def test_a_solve_after_every_stage_equals_the_fresh_solve():
    """The reverse direction in the same walk: the larger past, then every entry, then a solve."""
    want = fresh_outputs("solve")
    be = new_backend()
    try:
        hh.past_larger(be, "solve")
        for name, e in hh.ENTRIES.items():
            if name != "solve":
                e["fn"](be, hh.inputs("entry"))
        got = hh.ENTRIES["solve"]["fn"](be, hh.inputs("entry"))
    finally:
        be.close()
    assert_same(got, want, "solve after every stage")
