"""Stream continuation of the 40 MHz HT receive handle (sora_ht40_set_stream_mode, sora_ht40_stream_consumed), checked without a GPU: the built
library exports both entry points, the header declares them and the binding types them; a null handle is refused before any device work; and
RxHt40 carries the two methods the other three receive handles have."""
import ctypes

import pytest

from test_capi_cpu import declared_functions

NEW = ("sora_ht40_set_stream_mode", "sora_ht40_stream_consumed")
SORA_ERR_INVALID_PARAM = -1                                             # include/sora_hip.h


@pytest.fixture(scope="module")
def lib():
    import sora_amd
    return sora_amd.load(build_if_missing=False)


def test_library_exports_both_symbols(lib):
    from sora_amd import capi
    for n in NEW:
        assert hasattr(lib, n), "libsora_hip.so does not export %s" % n
        assert n in declared_functions() and n in capi.EXPORTS, n
        assert getattr(lib, n).argtypes is not None, n


def test_null_handle_is_refused_without_a_device(lib):
    lib.sora_hip_table_digest(None, None)                               # leaves a message that names no receive handle
    assert lib.sora_ht40_set_stream_mode(None, 1) == SORA_ERR_INVALID_PARAM
    assert b"sora_ht40_set_stream_mode" in lib.sora_hip_last_error()
    assert lib.sora_ht40_set_stream_mode(None, -1) == SORA_ERR_INVALID_PARAM
    assert lib.sora_ht40_stream_consumed(None, 0, None, 0) == SORA_ERR_INVALID_PARAM
    assert b"sora_ht40_stream_consumed" in lib.sora_hip_last_error()
    out = (ctypes.c_uint32 * 4)()
    assert lib.sora_ht40_stream_consumed(None, 1, ctypes.cast(out, ctypes.c_void_p), 4) == SORA_ERR_INVALID_PARAM


def test_rxht40_has_both_methods(lib):
    import sora_amd
    for name in ("set_stream_mode", "stream_consumed"):
        assert callable(getattr(sora_amd.RxHt40, name, None)), name
    # ... and they resolve to this handle's own entry points
    assert sora_amd.RxHt40._pre + "_set_stream_mode" == NEW[0] and sora_amd.RxHt40._pre + "_stream_consumed" == NEW[1]
