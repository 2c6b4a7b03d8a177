"""The marshalling layer of the ctypes binding (surfh_amd/_lib.py) against stub callables standing in for the C functions: what a
wrapper hands to a ``float *`` or a ``void *``, the callback trampoline with its exception path, and the two host-buffer solve
paths.  No GPU, no plan."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

from surfh_amd import _lib

MODEL = SimpleNamespace(_plan=C.c_void_p(1), isize=6, osize=4, ishape=(2, 3))
VALUES = np.arange(6, dtype=np.float64).reshape(2, 3) + 0.25


# ---- f32_vec, dev_ptr, seed64 ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,a", [
    ("list", VALUES.tolist()),
    ("float64", VALUES.copy()),
    ("fortran", np.asfortranarray(VALUES.astype(np.float32))),
    ("strided", np.repeat(VALUES.astype(np.float32), 2, axis=1)[:, ::2]),
    ("flat float32", VALUES.astype(np.float32).reshape(-1)),
])
def test_f32_vec_gives_the_flat_contiguous_float32_vector(name, a):
    v = _lib.f32_vec(a, 6, "six expected")
    assert isinstance(v, np.ndarray) and v.dtype == np.float32 and v.shape == (6,) and v.flags.c_contiguous
    assert np.array_equal(v, VALUES.astype(np.float32).reshape(-1))                     # in C order, whatever the layout was
    assert (name == "flat float32") == (isinstance(a, np.ndarray) and np.shares_memory(v, a))
    with pytest.raises(ValueError, match=r"^exactly this, 7 \(of 6\)$"):
        _lib.f32_vec(a, 7, "exactly this, 7 (of 6)")


def test_f32_vec_keeps_a_contiguous_float32_array_of_any_shape_in_place():
    a = VALUES.astype(np.float32)
    assert np.shares_memory(_lib.f32_vec(a, 6, "-"), a)


def test_f32_vec_passes_none_through_only_where_allowed():
    assert _lib.f32_vec(None, 6, "-", optional=True) is None
    with pytest.raises(ValueError, match="^no vector$"):
        _lib.f32_vec(None, 6, "no vector")
    with pytest.raises(ValueError, match="^wrong size$"):
        _lib.f32_vec(np.zeros(5), 6, "wrong size", optional=True)


def test_dev_ptr_takes_a_tensor_an_address_or_none():
    class Tensor:
        def data_ptr(self):
            return 0x7F0012345600

    for t, want in ((0x1000, 0x1000), (Tensor(), 0x7F0012345600), (2 ** 63 + 8, 2 ** 63 + 8)):
        p = _lib.dev_ptr(t)
        assert isinstance(p, C.c_void_p) and p.value == want
    assert _lib.dev_ptr(None) is None
    with pytest.raises(AttributeError):
        _lib.dev_ptr(1.5)


def test_seed64_keeps_the_low_64_bits():
    for seed, want in ((0, 0), (7, 7), (2 ** 64 + 5, 5), (-1, 2 ** 64 - 1), (np.int64(9), 9)):
        s = _lib.seed64(seed)
        assert isinstance(s, C.c_uint64) and s.value == want


# ---- the trampoline ----------------------------------------------------------------------------------------------------------------
TRACE = (3.0, 2.0, 1.0)
ITERATE = (0.5, 1.5, 2.5, 3.5, 4.5, 5.5)


def _c_arrays():
    return (C.c_double * 3)(*TRACE), (C.c_float * 6)(*ITERATE)


CB_TYPES = [(_lib.CG_CALLBACK, (2,), 2), (_lib.SAMPLE_CALLBACK, (7, 2), 7)]       # the C arguments before the trace, the callback's first


@pytest.mark.parametrize("cbtype,head,first", CB_TYPES)
def test_trampoline_hands_copies_to_the_callback(cbtype, head, first):
    trace, x = _c_arrays()
    seen = []

    def callback(it, g, xi):
        seen.append((it, g.copy(), xi.copy()))
        g[:] = -1.0                                                                      # copies: the library's arrays stay as they are
        xi[:] = -1.0
        return len(seen) == 2                                                            # falsy, then truthy

    cb, finish = _lib.trampoline(cbtype, callback, _lib.iterate_args(6, (2, 3)))
    assert cb(None, *head, trace, x) == 0 and cb(None, *head, trace, x) == 1
    assert tuple(trace) == TRACE and tuple(x) == ITERATE
    for it, g, xi in seen:
        assert it == first and g.dtype == np.float64 and np.array_equal(g, TRACE)
        assert xi.dtype == np.float64 and xi.shape == (2, 3) and np.array_equal(xi.reshape(-1), ITERATE)
    finish(0)                                                                            # nothing held, return code 0: nothing raised
    for truthy in (1, "stop", np.bool_(True)):
        assert _lib.trampoline(cbtype, lambda *a: truthy, _lib.iterate_args(6, (2, 3)))[0](None, *head, trace, x) == 1
    for falsy in (0, None, ""):
        assert _lib.trampoline(cbtype, lambda *a: falsy, _lib.iterate_args(6, (2, 3)))[0](None, *head, trace, x) == 0


def test_trampoline_trace_has_one_column_per_plane():
    trace, x = (C.c_double * 6)(1, 2, 3, 4, 5, 6), (C.c_float * 6)(*ITERATE)
    seen = []
    cb, _ = _lib.trampoline(_lib.CG_CALLBACK, lambda it, g, xi: seen.append(g), _lib.iterate_args(6, (6,), planes=2, squeeze=False))
    assert cb(None, 2, trace, x) == 0
    assert np.array_equal(seen[0], [[1, 2], [3, 4], [5, 6]])


@pytest.mark.parametrize("cbtype,head,first", CB_TYPES)
@pytest.mark.parametrize("raised", [KeyError, KeyboardInterrupt])
@pytest.mark.parametrize("rc", [0, 3])
def test_trampoline_holds_the_exception_and_raises_it_before_the_return_code(cbtype, head, first, raised, rc):
    trace, x = _c_arrays()

    def callback(it, g, xi):
        raise raised("from the callback")

    cb, finish = _lib.trampoline(cbtype, callback, _lib.iterate_args(6, (2, 3)))
    assert cb(None, *head, trace, x) == 1                                               # held: the library is told to stop
    with pytest.raises(raised, match="from the callback"):
        finish(rc, ValueError)


def test_trampoline_without_a_callback_is_the_null_pointer_and_finish_checks_the_code():
    cb, finish = _lib.trampoline(_lib.CG_CALLBACK, None, None)
    assert not cb
    finish(0)
    for exc in (RuntimeError, ValueError):
        with pytest.raises(exc):
            finish(1, exc)


# ---- _solve ------------------------------------------------------------------------------------------------------------------------
def _solver_stub(n_lead, stop_at, planes=1, size=6, rc=0, log=None):
    """``fn(plan, y, *lead, x0, max_iter, tol, refresh, x, grad_norm, nit, *outs, callback, user)``: iteration ``it`` writes
    ``x = x0 + it`` and ``grad_norm[it, l] = 10 it + l``, calls the callback, stops after ``stop_at`` iterations or on its word."""
    def fn(plan, y, *args):
        lead, (x0, max_iter, tol, refresh, x, gn, nit), rest = args[:n_lead], args[n_lead:n_lead + 7], args[n_lead + 7:]
        cb = rest[-2]
        if log is not None:
            log.update(plan=plan, y=np.ctypeslib.as_array(y, shape=(MODEL.osize,)).copy(), lead=lead, x0=x0, max_iter=max_iter, tol=tol,
                       refresh=refresh, outs=rest[:-2], user=rest[-1])
        xa = np.ctypeslib.as_array(x, shape=(size,))
        ga = np.ctypeslib.as_array(gn, shape=(max_iter + 1, planes))
        start = 0.0 if x0 is None else np.ctypeslib.as_array(x0, shape=(size,))
        xa[:] = start
        ga[0] = np.arange(planes)
        it = 0
        while it < min(stop_at, max_iter):
            it += 1
            xa[:] = start + it
            ga[it] = 10 * it + np.arange(planes)
            if cb and cb(None, it, gn, x):
                break
        nit._obj.value = it
        return rc
    return fn


def test_solve_trims_and_shapes_the_trace():
    log = {}
    x, gn, nit = _lib.solve(MODEL, _solver_stub(2, 3, log=log), [1, 2, 3, 4], 2, 0.5, None, 8, 1e-3, 5, None)
    assert nit == 3 and x.dtype == np.float64 and x.shape == (2, 3) and np.all(x == 3.0)
    assert gn.shape == (4,) and np.array_equal(gn, [0, 10, 20, 30])                    # [nit+1], squeezed for a single image
    assert log["plan"] is MODEL._plan and np.array_equal(log["y"], [1, 2, 3, 4]) and log["lead"] == (2.0, 0.5) and log["x0"] is None
    assert (log["max_iter"], log["tol"], log["refresh"], log["outs"], log["user"]) == (8, 1e-3, 5, (), None)
    x, gn, nit = _lib.solve(MODEL, _solver_stub(2, 9, planes=3), np.zeros(4), 1, 0, VALUES, 2, 0, 5, None, planes=3, squeeze=False)
    assert nit == 2 and np.array_equal(x, VALUES + 2)                                    # from x0, stopped by max_iter
    assert gn.shape == (3, 3) and np.array_equal(gn, [[0, 1, 2], [10, 11, 12], [20, 21, 22]])
    _, gn, nit = _lib.solve(MODEL, _solver_stub(2, 0), np.zeros(4), 1, 0, None, 4, 0, 5, None)
    assert nit == 0 and gn.shape == (1,)


def test_solve_size_errors_keep_their_messages():
    fn = _solver_stub(2, 1)
    with pytest.raises(ValueError, match="^data size mismatch$"):
        _lib.solve(MODEL, fn, np.zeros(5), 1, 0, None, 2, 0, 5, None)
    with pytest.raises(ValueError, match="^x0 size mismatch$"):
        _lib.solve(MODEL, fn, np.zeros(4), 1, 0, np.zeros(5), 2, 0, 5, None)
    with pytest.raises(ValueError, match="^x0 size mismatch$"):                         # against the iterate's own size where one is given
        _lib._solve(MODEL, fn, np.zeros(4), (1, 0), np.zeros(6), 2, 0, 5, (), None, size=8, shape=(2, 4))


def test_solve_callback_stops_and_sees_the_custom_iterate_shape():
    """What ``cg_templates`` asks of ``_solve``: a pointer among the leading arguments, an iterate that is not the model's."""
    seen, log = [], {}
    maps = np.ones(6, dtype=np.float32)

    def callback(it, g, s):
        seen.append((it, g, s))
        return it == 2

    S, gn, nit = _lib._solve(MODEL, _solver_stub(3, 9, size=8, log=log), np.zeros(4), (_lib.fptr(maps), 2, 3), None, 5, 0, 5, (), callback,
                             size=8, shape=(2, 4), exc=ValueError)
    assert nit == 2 and S.shape == (2, 4) and np.all(S == 2.0) and np.array_equal(gn, [0, 10, 20])
    assert isinstance(log["lead"][0], _lib.c_float_p) and log["lead"][1:] == (2.0, 3.0)
    assert [(it, g.tolist(), s.shape, float(s[0, 0])) for it, g, s in seen] == [(1, [0, 10], (2, 4), 1.0), (2, [0, 10, 20], (2, 4), 2.0)]


@pytest.mark.parametrize("rc", [0, 3])
def test_solve_raises_the_callbacks_exception_after_the_library_returns(rc):
    calls = []

    def callback(it, g, x):
        calls.append(it)
        if it == 2:
            raise KeyError("second call")

    with pytest.raises(KeyError, match="second call"):
        _lib.solve(MODEL, _solver_stub(2, 9, rc=rc), np.zeros(4), 1, 0, None, 5, 0, 5, callback)
    assert calls == [1, 2]                                                               # the loop stopped there
    with pytest.raises(ValueError):                                                      # no exception held: the code, as ``exc``
        _lib._solve(MODEL, _solver_stub(2, 1, rc=3), np.zeros(4), (1, 0), None, 5, 0, 5, (), None, exc=ValueError)


def test_solve_huber_planes_has_one_implementation_behind_both_names(monkeypatch):
    got = []

    def fake(model, fn, data, lead, *rest):
        got.append((fn, lead))
        return ("x", "gn", 1)

    lib = SimpleNamespace(surfh_mmmg_huber_planes="scalar", surfh_mmmg_huber_planes_ex="ex")
    monkeypatch.setattr(_lib, "load", lambda: lib)
    monkeypatch.setattr(_lib, "_solve", fake)
    r, d = np.array([1.0, 2.0]), np.array([0.1, 0.2])
    out = _lib.solve_huber_planes(MODEL, None, 3, 1.5, 0.25, None, 5, 0, 5, None, 2, False)
    assert out[:3] == ("x", "gn", 1) and out[3].shape == (2,)
    assert got[-1] == ("scalar", (3, 1.5, 0.25))                                         # numbers, left to the library to check
    for call in (lambda: _lib.solve_huber_planes_ex(MODEL, None, 3, r, d, 1, None, 5, 0, 5, None, 2, False),
                 lambda: _lib.solve_huber_planes(MODEL, None, 3, r, d, None, 5, 0, 5, None, 2, False, coupling=1)):
        call()
        fn, lead = got[-1]
        assert fn == "ex" and lead[0] == 3 and isinstance(lead[3], C.c_int32) and lead[3].value == 1
        assert [np.ctypeslib.as_array(p, shape=(2,)).tolist() for p in lead[1:3]] == [r.tolist(), d.tolist()]


# ---- _solve_nonneg -----------------------------------------------------------------------------------------------------------------
def _admm_stub(n_lead, stop_at, planes=None, size=6, rc=0, log=None):
    """``fn(plan, y, *lead, start, outer, inner, tol, refresh, out, trace, nit)``: fills ``trace[k, j(, l)] = 100 k + 10 j (+ l)``."""
    def fn(plan, y, *args):
        lead, (start, outer, inner, tol, refresh, out, trace, nit) = args[:n_lead], args[n_lead:]
        if log is not None:
            log.update(lead=lead, start=start, outer=outer, inner=inner, tol=tol, refresh=refresh)
        shape = (outer + 1, 4) + (() if planes is None else (planes,))
        t = np.ctypeslib.as_array(trace, shape=shape)
        k, j = np.arange(outer + 1), np.arange(4)
        t[...] = (100 * k[:, None] + 10 * j[None, :]) if planes is None else (100 * k[:, None, None] + 10 * j[None, :, None] + np.arange(planes))
        np.ctypeslib.as_array(out, shape=(size,))[:] = 7.0 if start is None else np.ctypeslib.as_array(start, shape=(size,)) + 1
        nit._obj.value = min(stop_at, outer)
        return rc
    return fn


def test_solve_nonneg_single_trace():
    log = {}
    x, trace, nit = _lib._solve_nonneg(MODEL, _admm_stub(3, 2, log=log), np.zeros(4), (1, 0.5, 2), None, 5, 3, 1e-4, 2)
    assert nit == 2 and x.dtype == np.float64 and x.shape == (2, 3) and np.all(x == 7.0)
    assert trace.shape == (6, 4) and trace.dtype == np.float64 and trace[2, 3] == 230.0
    assert log == dict(lead=(1.0, 0.5, 2.0), start=None, outer=5, inner=3, tol=1e-4, refresh=2)
    from surfh_amd.nonneg import result_from_trace
    r = result_from_trace(x, trace, 2.0, nit)
    assert r.primal.shape == (3,) and np.array_equal(r.n_active, [30, 130, 230]) and r.nit == 2


def test_solve_nonneg_plane_wise_trace_and_custom_size():
    rho = np.array([1.0, 2.0, 3.0])
    x, trace, nit = _lib._solve_nonneg(MODEL, _admm_stub(3, 9, planes=3), np.zeros(4), (1, 0, _lib.dptr(rho)), VALUES, 2, 1, 0, 0, planes=3)
    assert nit == 2 and np.array_equal(x, VALUES + 1)
    assert trace.shape == (3, 4, 3) and trace[1, 2, 1] == 121.0
    from surfh_amd.nonneg import result_from_planes_trace
    r = result_from_planes_trace(x, trace, rho, nit)
    assert r.grad_norm.shape == (3, 3) and np.array_equal(r.n_active[2], [230, 231, 232])
    S, trace, nit = _lib._solve_nonneg(MODEL, _admm_stub(4, 1, size=8), np.zeros(4), (_lib.fptr(np.ones(6, dtype=np.float32)), 1, 0, 2),
                                       np.zeros(8, dtype=np.float32), 1, 1, 0, 0, size=8, shape=(2, 4))
    assert S.shape == (2, 4) and np.all(S == 1.0) and trace.shape == (2, 4) and nit == 1


def test_solve_nonneg_errors():
    with pytest.raises(ValueError, match="^data size mismatch$"):
        _lib._solve_nonneg(MODEL, _admm_stub(3, 1), np.zeros(3), (1, 0, 1), None, 1, 1, 0, 0)
    with pytest.raises(ValueError, match="^x0 size mismatch$"):
        _lib._solve_nonneg(MODEL, _admm_stub(3, 1), np.zeros(4), (1, 0, 1), np.zeros(5), 1, 1, 0, 0)
    with pytest.raises(ValueError):                                                      # the library's refusals are ValueError
        _lib._solve_nonneg(MODEL, _admm_stub(3, 1, rc=1), np.zeros(4), (1, 0, 1), None, 1, 1, 0, 0)


# ---- PlanOwner ---------------------------------------------------------------------------------------------------------------------
def test_plan_owner_is_the_one_home_of_the_life_cycle():
    from surfh_amd.blurred2d import Blurred2D
    from surfh_amd.models import spectroSigRLSCT
    from surfh_amd.plan_owner import PlanOwner
    from surfh_amd.spectro_blind import MRSBlurred
    for name in ("__del__", "stream", "_host", "forward_dev", "adjoint_dev", "adjoint_ref_dev", "fwadj_dev", "profile_enable",
                 "profile_filter", "profile_reset", "profile"):
        for cls in (spectroSigRLSCT, Blurred2D, MRSBlurred):
            assert getattr(cls, name) is getattr(PlanOwner, name), (cls, name)
    assert Blurred2D.close is PlanOwner.close and spectroSigRLSCT.close is not PlanOwner.close       # its channels' plans first
    destroyed = []

    class Owner(PlanOwner):
        def __init__(self):
            self._L, self._plan = SimpleNamespace(surfh_plan_destroy=destroyed.append), C.c_void_p(5)

    o = Owner()
    o.close()
    o.close()
    assert [p.value for p in destroyed] == [5] and o._plan is None
    PlanOwner().close()                                                                  # never had a plan: nothing to destroy
    out = PlanOwner._host(SimpleNamespace(_plan=None), lambda plan, a, b: 0, VALUES, 6, (3, 2))
    assert out.shape == (3, 2) and out.dtype == np.float64
    with pytest.raises(ValueError, match="^input has 6 elements, expected 5$"):
        PlanOwner._host(SimpleNamespace(_plan=None), None, VALUES, 5, (5,))
