"""ABI surface of the lean solve-kernel instance, checked without a device: the header declares `omgx_batch_last_instance` behind
OMGX_HAS_LAST_INSTANCE, the library exports it, the ABI version is still 9, a null handle is refused; and the header states the
contract of `omgx_batch_set_stop` the lean / full comparison of tests/test_gpu_lean_instance.py relies on -- a negative tolerance is
a rule that never holds (`stop_criterium`: two Euclidean norms <= stop_tol), which the host executor's `arrived` obeys too."""
import ctypes
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_surface_of_the_instance_query():
    from omgtools.backend import LIB_PATH
    header = open(os.path.join(ROOT, 'include', 'omgx.h')).read()
    assert re.search(r'#define\s+OMGX_HAS_LAST_INSTANCE\s+1\b', header) and re.search(r'#define\s+OMGX_VERSION\s+9\b', header)
    assert re.search(r'\bint\s+omgx_batch_last_instance\s*\(\s*const\s+omgx_batch\s*\*', header)
    lib = ctypes.CDLL(LIB_PATH)
    lib.omgx_version.restype = ctypes.c_int
    assert lib.omgx_version() == 9
    assert hasattr(lib, 'omgx_batch_last_instance')
    lib.omgx_batch_last_instance.argtypes = [ctypes.c_void_p]
    lib.omgx_batch_last_instance.restype = ctypes.c_int
    assert lib.omgx_batch_last_instance(None) == -1                  # OMGX_E_INVALID
    lib.omgx_batch_set_stop.argtypes = [ctypes.c_void_p] + [ctypes.c_int32] * 4 + [ctypes.c_double, ctypes.c_void_p]
    assert lib.omgx_batch_set_stop(None, 0, 0, 0, 1, -1.0, None) == -1


def test_a_negative_stop_tolerance_is_documented_and_never_holds_on_the_host_executor():
    """Without a device there is no handle, and `omgx_batch_set_stop` refuses a null handle before it looks at the tolerance: the
    library's own validation is exercised on a real handle by tests/test_gpu_lean_instance.py.  Here: the header states the contract,
    and the host executor's statement of the criterion (`BatchP2P.arrived`) obeys it."""
    header = open(os.path.join(ROOT, 'include', 'omgx.h')).read()
    assert 'A negative stop_tol is a rule that never holds' in header
    from omgtools.batch import BatchP2P

    class _Stub(object):
        o_state0, o_input0, n_dim = 0, 2, 2
        p = np.zeros((3, 6))                                         # state == target, input == 0: arrived at any tolerance >= 0
        _o_pose = lambda self, who, point_mass=True: 4
        _norm = staticmethod(lambda a: np.linalg.norm(a, axis=1))
    assert BatchP2P.arrived(_Stub(), 0.0).all()
    assert not BatchP2P.arrived(_Stub(), -1.0).any()
    assert not BatchP2P.arrived(_Stub(), -np.inf).any()
