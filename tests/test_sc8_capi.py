"""CPU checks of the 8-bit I/Q boundary (no GPU compute is called): the row-table OFDM call is
exported and refuses a null handle, the queue takes format 2 as a format (a null queue is still
refused), and the headers give SRSGPU_RXQ_SC8 and SRSGPU_SAMPLES_SC8 the same value."""
import ctypes
import os
import re

from conftest import REPO

LIB = os.path.join(REPO, "empower-srslte_amd", "lib", "libsrsgpu_phy.so")


def _define(header, name):
    src = open(os.path.join(REPO, "include", "srsgpu", header)).read()
    m = re.search(r"^#define\s+%s\s+(\d+)\b" % name, src, flags=re.M)
    assert m, (header, name)
    return int(m.group(1))


def test_rows_call_is_exported_and_refuses_a_null_handle():
    lib = ctypes.CDLL(LIB)
    assert hasattr(lib, "srsgpu_ofdm_rx_sf_rows_dev")
    f = lib.srsgpu_ofdm_rx_sf_rows_dev
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_float,
                  ctypes.c_void_p, ctypes.c_size_t]
    buf = (ctypes.c_uint8 * 64)()
    assert f(None, 1, buf, 2, 1.0, buf, 1 << 20) == -1


def test_queue_refuses_sc8_without_a_queue():
    lib = ctypes.CDLL(LIB)
    lib.srsgpu_rxq_set_input_format.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_float]
    assert lib.srsgpu_rxq_set_input_format(None, 2, 0.0) == -1


def test_headers_define_the_formats():
    assert _define("rx_queue.h", "SRSGPU_RXQ_SC8") == 2
    assert _define("ofdm_batch.h", "SRSGPU_SAMPLES_SC8") == 2
    # the queue's formats are the OFDM call's: one set of values
    for q, o in (("SRSGPU_RXQ_CF32", "SRSGPU_SAMPLES_CF32"), ("SRSGPU_RXQ_SC16", "SRSGPU_SAMPLES_SC16")):
        assert _define("rx_queue.h", q) == _define("ofdm_batch.h", o)


def test_python_mirror_has_the_format_and_the_call():
    import srsgpu_phy as s
    assert s.RxQueue.SC8 == 2 and s.RxQueue.SC16 == 1 and s.RxQueue.CF32 == 0
    assert "srsgpu_ofdm_rx_sf_rows_dev" in s.EXPORTED
    assert callable(s.OfdmRx.rx_rows_dev)
