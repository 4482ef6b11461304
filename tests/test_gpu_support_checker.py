"""No GPU: the two asserting helpers of tests/gpu_support.py can fail.  assert_reader_refusals runs against stub handles whose reader
answers as mfr::prepare does, then with one answer spoiled at a time; code_of against calls that raise, raise something else, or return."""
import pytest

from cortex.jl_amd import _lib as L
from tests import gpu_support as GS

WHO, SMALL = "cx_reader_mfma", "cx_reader"
ANSWERS = {      # case -> (code, the words of mfr::prepare behind "who: ")
    "small dim": (L.ERR_UNSUPPORTED, "the matrix-core dims, 5 .. 64 (dim 1, 2, 3 and 4: cx_reader)"),
    "natural2": (L.ERR_UNSUPPORTED, "the Gaussian family only (no such thing)"),
    "structured vmp": (L.ERR_UNSUPPORTED, "the Gaussian family only (no such thing)"),
    "no graph": (L.ERR_STATE, "no graph"),
    "state halo": (L.ERR_UNSUPPORTED, "not for a partitioned handle (halo lists, state halos or a chain's time block: its rows would need owners)"),
    "a time block now": (L.ERR_UNSUPPORTED, "not for a partitioned handle (halo lists, state halos or a chain's time block: its rows would need owners)"),
    "captured": (L.ERR_STATE, "the handle's stream is being captured (the call is synchronous)"),
    "never set": (L.ERR_STATE, "parameter set 1 was never set (cx_set_factor_matrices)"),
}


class _Handle:
    def __init__(self, case):
        self.case = case

    def halo_configure(self, *lists):
        assert self.case == "time block"
        self.case = "a time block now"

    def close(self):
        pass


class _Rig:
    """stub handles; the stub raw call already returns what under_capture returns: (status, last error)"""
    device = staticmethod(_Handle)

    @staticmethod
    def under_capture(dev, call):
        return call()


def _run(spoil=None, **kw):
    """assert_reader_refusals on the stubs; spoil = (case, code, message) replaces that case's answer"""
    answers = {k: (c, f"{WHO}: {m}") for k, (c, m) in ANSWERS.items()}
    if spoil is not None:
        answers[spoil[0]] = spoil[1:]

    def call(dev):
        if dev.case in answers:
            raise L.CortexHipError(*answers[dev.case])

    def small_call(dev):
        assert dev.case == "small call"
        raise L.CortexHipError(*answers.get("small call", (L.ERR_UNSUPPORTED, f"{SMALL}: dim 1 .. 4")))

    GS.assert_reader_refusals(WHO, SMALL, call, small_call, lambda dev: answers["captured"], rig=_Rig, **kw)


def test_a_reader_that_answers_as_mfr_prepare_does_passes():
    _run()
    _run(cases=GS.HANDLE_CASES)
    _run(cases=GS.STREAM_CASES)


@pytest.mark.parametrize("case", sorted(ANSWERS))
def test_a_wrong_code_fails(case):
    code, msg = ANSWERS[case]
    with pytest.raises(AssertionError):
        _run((case, L.ERR_INVALID_ARGUMENT, f"{WHO}: {msg}"))


@pytest.mark.parametrize("case", sorted(ANSWERS))
def test_a_message_under_another_calls_name_fails(case):
    code, msg = ANSWERS[case]
    with pytest.raises(AssertionError):
        _run((case, code, f"cx_other_mfma: {msg}"))
    with pytest.raises(AssertionError):
        _run((case, code, f"{WHO}_rows: {msg}"))      # a longer name that begins with the reader's


@pytest.mark.parametrize("case", sorted(ANSWERS))
def test_a_message_without_the_expected_words_fails(case):
    code, _ = ANSWERS[case]
    with pytest.raises(AssertionError):
        _run((case, code, f"{WHO}: refused"))


def test_the_small_call_must_keep_refusing_and_the_small_name_must_be_named():
    with pytest.raises(AssertionError):
        _run(("small call", L.ERR_STATE, f"{SMALL}: something else"))
    with pytest.raises(AssertionError):      # "cx_reader" only as the head of the reader's own name
        _run(("small dim", L.ERR_UNSUPPORTED, f"{WHO}: the matrix-core dims, 5 .. 64"))


def test_a_skipped_case_is_not_asked_and_an_unknown_one_is_refused():
    _run(("no graph", L.OK, "nothing"), skip=("no graph",))
    with pytest.raises(AssertionError):
        _run(skip=("no such case",))


def test_code_of():
    def refuse(code, text):
        raise L.CortexHipError(code, text)

    assert GS.code_of(refuse, L.ERR_STATE, text="no graph") == (L.ERR_STATE, "no graph")
    with pytest.raises(ValueError):
        GS.code_of(lambda: int("x"))                  # another exception passes through
    with pytest.raises(pytest.fail.Exception):
        GS.code_of(lambda: None)                      # a call that does not raise fails the test
