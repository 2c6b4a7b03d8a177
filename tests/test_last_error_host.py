"""surfh_last_error() across the four host files of the plan library.  The error string has one definition, in plan.hip beside
fail(); plan_ops.hip, plan_solvers.hip and plan_diag.hip raise their errors through the declaration in plan_internal.h.  A copy of
the string per file would leave surfh_last_error() empty, or stale, for every failure raised outside plan.hip.  Each call below
fails in its entry point's argument check, before anything touches a device.  No GPU."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    ge.build()
    from surfh_amd import _lib
    return _lib.load()


def _mmmg(lib):
    from surfh_amd import _lib
    return lib.surfh_mmmg(None, None, 1.0, 0.0, None, 1, 0.0, 0, None, None, None, _lib.CG_CALLBACK(0), None)


# (file that raises the error, the failing call, the words of its message)
CALLS = [
    ("plan.hip", lambda L: L.surfh_plan_create(None, None), "null argument"),
    ("plan_ops.hip", lambda L: L.surfh_forward_dev(None, None, None), "null plan"),
    ("plan_solvers.hip", _mmmg, "null argument"),
    ("plan_diag.hip", lambda L: L.surfh_profile_enable(None, 1), "null plan"),
    ("plan_diag.hip", lambda L: L.surfh_mm_step2(1.0, 0.0, 1.0, 1.0, 0.0, None), "null argument"),
    ("plan_ops.hip", lambda L: L.surfh_normal_dev(None, None, None, 1.0), "null plan"),
]


def test_every_file_reports_through_the_one_error_string(lib):
    for where, call, words in CALLS:
        assert lib.surfh_get_potential(None, 7) == -1          # a message of plan.hip that none of the calls produces
        assert "slot 7" in lib.surfh_last_error().decode()
        assert call(lib) != 0, where
        assert lib.surfh_last_error().decode() == words, (where, lib.surfh_last_error())
    # without the reset in between: neighbouring calls come from different files and carry different messages, so a stale
    # string would show the previous one
    for where, call, words in CALLS:
        assert call(lib) != 0, where
        assert lib.surfh_last_error().decode() == words, (where, lib.surfh_last_error())
