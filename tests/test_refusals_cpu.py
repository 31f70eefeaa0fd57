"""Bad handle lists on the CPU oracle: the oracle half of tests/test_refusals_gpu.py.

Every list of tests/refusals_lib.LISTS goes to every control call the oracle
exports, after the 2-second configs[0] trace has run and one DownTrack has
been removed.  The oracle's return code must be the one include/lkfwd.h
documents (refusals_lib.CONTRACT), a refused call must leave every DownTrack's
state as it was, and the cases where the engine's answer is pinned instead of
compared may be no more than one in ten."""
import ctypes as C

from tests import refusals_lib as R


def _states(abi, api, h, ndts):
    out = []
    for d in range(ndts):
        st = abi.lkf_fwd_state()
        assert api["get_state"](h, d, C.byref(st)) == 0
        out.append(st.as_tuple())
    return out


def test_pins_are_at_most_one_case_in_ten():
    assert 10 * len(R.pinned_cases()) <= R.total_cases(), (len(R.pinned_cases()), R.total_cases())
    for name, which in R.pinned_cases():
        assert name in R.CONTRACT and which in R.LISTS and name not in R.NO_ORACLE


def test_oracle_answers_follow_the_header(workload, abi, oracle):
    tr, oh = R.forwarded_oracle(workload, oracle)
    try:
        handles = R.prepare(oracle.api, oh, tr)
        before = _states(abi, oracle.api, oh, tr.ndts)
        got = R.oracle_answers(oracle, oh, handles)
        assert len(got) == R.total_cases() - len(R.NO_ORACLE) * len(R.LISTS) - len(R.PINNED_CODES)
        for (name, which), (rc, counts, _) in got.items():
            print(name, which, rc, counts)
            assert rc == R.contract_code(name, which), (name, which, rc)
            if rc != R.OK and (name, which) not in R.PINNED_COUNTS and name != "rtx_lookup":
                assert all(c == R.SENT for c in counts), (name, which, counts)  # a refusal writes no count
        for which in R.LISTS:  # (lkf_rtx_lookup: *n_out = 0 first, on both sides)
            if got[("rtx_lookup", which)][0] != R.OK:
                assert got[("rtx_lookup", which)][1] == (0,)
        assert _states(abi, oracle.api, oh, tr.ndts) == before
    finally:
        oracle.destroy(oh)
        tr.close()
