"""CPU: "the last failure on the calling thread is lzx_last_error()" (include/lzx.h, conventions) with more than one thread.
Argument errors return before the device is touched (as in test_trace_host.py), and ctypes.CDLL releases the GIL around every
call, so the failing calls below really overlap."""
import ctypes
import threading

import numpy as np

_f64p = ctypes.POINTER(ctypes.c_double)
LZX_ERR_ARG = -1


def test_last_error_belongs_to_the_calling_thread(pkg):
    """Three threads behind one barrier: A fails lzx_spmm_f64 with a null handle, B fails lzx_probes_f64 with a null handle, C
    fails nothing.  After a second barrier each reads lzx_last_error(): A sees its own function's name and not B's, B its own
    and not A's, C neither.  The main thread's own earlier failure is still there when they are done."""
    L = pkg.lib()
    x, y = np.zeros(64), np.zeros(64)
    assert L.lzx_probe_diag_f64(None, x.ctypes.data_as(_f64p), 4, y.ctypes.data_as(_f64p)) == LZX_ERR_ARG
    barrier = threading.Barrier(3)
    seen, errors = {}, {}

    def body(role):
        try:
            a, b = np.zeros(64), np.zeros(64)
            barrier.wait(timeout=30)
            rc = 0
            if role == "A":
                rc = L.lzx_spmm_f64(None, 2, a.ctypes.data_as(_f64p), b.ctypes.data_as(_f64p))
            elif role == "B":
                rc = L.lzx_probes_f64(None, 1, 0, 2, a.ctypes.data_as(_f64p))
            barrier.wait(timeout=30)
            seen[role] = (rc, L.lzx_last_error().decode())
        except BaseException as e:          # reported by the main thread, with the role's name
            errors[role] = e
            barrier.abort()

    threads = [threading.Thread(target=body, args=(r,), daemon=True) for r in "ABC"]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=60)
    assert not [t for t in threads if t.is_alive()]
    for role, e in errors.items():
        raise AssertionError(f"thread {role}: {e!r}") from e
    assert seen["A"][0] == LZX_ERR_ARG and "lzx_spmm_f64" in seen["A"][1] and "lzx_probes_f64" not in seen["A"][1], seen
    assert seen["B"][0] == LZX_ERR_ARG and "lzx_probes_f64" in seen["B"][1] and "lzx_spmm_f64" not in seen["B"][1], seen
    assert seen["C"][0] == 0 and "lzx_spmm_f64" not in seen["C"][1] and "lzx_probes_f64" not in seen["C"][1], seen
    assert "lzx_probe_diag_f64" not in seen["A"][1] + seen["B"][1] + seen["C"][1], seen
    assert "lzx_probe_diag_f64" in L.lzx_last_error().decode()
