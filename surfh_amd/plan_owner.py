"""``PlanOwner``: what every model that owns a plan of the library (``surfh_plan_create`` ... ``surfh_plan_destroy``) shares -- the
plan's life cycle, the host call helper, the operator on device pointers and the HIP-event profile."""
from __future__ import annotations

import ctypes as C

from . import _lib
from ._lib import dev_ptr


class PlanOwner:
    """Holds the loaded library ``_L`` and the plan ``_plan`` (set by the subclass once ``surfh_plan_create`` succeeded; ``None``
    before that and after ``close``).  The mixins ``DataWeights``, ``Potentials``, ``TemplateOps`` and ``NonnegOps`` act on one."""
    _L = None
    _plan = None

    # ---- life cycle -----------------------------------------------------------------------
    def close(self):
        if self._plan:
            self._L.surfh_plan_destroy(self._plan)
            self._plan = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def stream(self) -> int:
        return int(self._L.surfh_stream(self._plan) or 0)

    # ---- host arrays ----------------------------------------------------------------------
    def _host(self, fn, x, nin, shape_out):
        return _lib.host_call(fn, self._plan, x, nin, shape_out)

    # ---- device pointers (asynchronous on self.stream) ------------------------------------
    def forward_dev(self, x_t, y_t):
        _lib.check(self._L.surfh_forward_dev(self._plan, dev_ptr(x_t), dev_ptr(y_t)))

    def adjoint_dev(self, y_t, x_t):
        _lib.check(self._L.surfh_adjoint_dev(self._plan, dev_ptr(y_t), dev_ptr(x_t)))

    def adjoint_ref_dev(self, y_t, x_t):
        _lib.check(self._L.surfh_adjoint_ref_dev(self._plan, dev_ptr(y_t), dev_ptr(x_t)))

    def fwadj_dev(self, x_t, out_t):
        _lib.check(self._L.surfh_fwadj_dev(self._plan, dev_ptr(x_t), dev_ptr(out_t)))

    # ---- instrumentation ------------------------------------------------------------------
    def profile_filter(self, prefix=None):
        """Time only the stages whose name starts with ``prefix`` (None: all)."""
        _lib.check(self._L.surfh_profile_filter(self._plan, prefix.encode() if prefix else None))

    def profile_enable(self, on=True):
        _lib.check(self._L.surfh_profile_enable(self._plan, 1 if on else 0))

    def profile_reset(self):
        _lib.check(self._L.surfh_profile_reset(self._plan))

    def profile(self) -> dict:
        """{kernel name: (launches, total ms)} measured with HIP events on the plan's stream."""
        out = {}
        for i in range(self._L.surfh_profile_count(self._plan)):
            name, cnt, ms = C.c_char_p(), C.c_int64(), C.c_double()
            _lib.check(self._L.surfh_profile_get(self._plan, i, C.byref(name), C.byref(cnt), C.byref(ms)))
            out[name.value.decode()] = (cnt.value, ms.value)
        return out
