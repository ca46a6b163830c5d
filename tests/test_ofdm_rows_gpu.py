"""srsgpu_ofdm_rx_sf_rows_dev: the OFDM receive FFT from a table of raw rows, integer samples converted
in the FFT's first load. The comparison target is always the existing strided call,
srsgpu_ofdm_rx_sf_dev, on the host-converted floats v.astype(float32) * float32(scale): everything
after the load is the same kernel code, so the grids must be the same bits (compared as uint32, no
tolerance). A wrong address, a missing sign extension or a multiply contracted into the first
butterfly's add would all show as different bits."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SC16, SC8 = 1, 2
DTYPE = {SC16: np.int16, SC8: np.int8}
DEFAULT_SCALE = {SC16: 1.0 / 32768.0, SC8: 1.0 / 128.0}
ODD_SCALE = 3.1e-5  # no power of two: value * scale is inexact, so its rounding is observable


def _symbol_start(N, cp, slot, l):
    """first sample of symbol l of a slot (after its cyclic prefix)"""
    if cp:
        cp0 = cpn = -(-512 * N // 2048)
    else:
        cp0, cpn = -(-160 * N // 2048), -(-144 * N // 2048)
    return slot * (15 * N // 2) + cp0 + l * (N + cpn)


def _int_rows(rng, fmt, N, n, cp=0):
    """n subframes of uniformly random full-range integers [n, 15 N, 2], the extremes forced at the first
    and last sample of every row and around a symbol start"""
    ii = np.iinfo(DTYPE[fmt])
    v = rng.integers(ii.min, ii.max + 1, size=(n, 15 * N, 2), dtype=DTYPE[fmt])
    s1 = _symbol_start(N, cp, 0, 1)
    s2 = _symbol_start(N, cp, 1, 3)
    for at, val in ((0, (ii.min, ii.max)), (15 * N - 1, (ii.max, ii.min)), (s1 - 1, (ii.max, ii.max)),
                    (s1, (ii.min, ii.min)), (s1 + 1, (ii.max, ii.min)), (s2, (ii.min, ii.max)),
                    (s2 + N - 1, (ii.min, ii.min))):
        v[:, at] = val
    return v


def _scattered(torch, rng, rows, order):
    """the rows (equal-sized arrays) in one device buffer in the given order, junk gaps of 16-byte
    multiples before, between and after them; returns (buffer, device table of row pointers)"""
    nbytes = rows[0].nbytes
    assert nbytes % 16 == 0
    gaps = [16 * int(g) for g in rng.integers(1, 40, size=len(rows) + 1)]
    host = rng.integers(0, 256, size=sum(gaps) + len(rows) * nbytes, dtype=np.uint8)
    off, pos = [0] * len(rows), 0
    for k, r in enumerate(order):
        pos += gaps[k]
        off[r] = pos
        host[pos:pos + nbytes] = rows[r].reshape(-1).view(np.uint8)
        pos += nbytes
    d_buf = torch.from_numpy(host).cuda()
    assert d_buf.data_ptr() % 16 == 0
    d_tab = torch.tensor([d_buf.data_ptr() + o for o in off], dtype=torch.int64, device="cuda")
    return d_buf, d_tab


def _strided(torch, o, x, gsz):
    """the existing call on complex64 rows x [n, 15 N]: the grids as uint32"""
    n = x.shape[0]
    d_x = torch.from_numpy(np.ascontiguousarray(x).reshape(-1)).cuda()
    d_g = torch.zeros(n * gsz, dtype=torch.complex64, device="cuda")
    assert o.rx_dev(n, d_x.data_ptr(), x.shape[1], d_g.data_ptr(), gsz) == 0
    torch.cuda.synchronize()
    return d_g.cpu().numpy().view(np.uint32)


def _from_rows(torch, o, d_tab, n, fmt, scale, gsz):
    d_g = torch.zeros(n * gsz, dtype=torch.complex64, device="cuda")
    assert o.rx_rows_dev(n, d_tab.data_ptr(), fmt, scale, d_g.data_ptr(), gsz) == 0
    torch.cuda.synchronize()
    return d_g.cpu().numpy().view(np.uint32)


def _host_floats(v, scale):
    return (v.astype(np.float32) * np.float32(scale)).view(np.complex64)[..., 0]


@pytest.mark.parametrize("fmt", [SC8, SC16])
@pytest.mark.parametrize("nof_prb,N", [(6, 128), (25, 384), (25, 512), (100, 1536), (100, 2048), (75, 1152)])
def test_integer_rows_equal_converted_floats(nof_prb, N, fmt):
    """SC8 and SC16 rows, scattered in scrambled order between junk, at the LTE sizes (several symbols
    per workgroup, one per workgroup, radix 3) and a size of the run-time-planned kernel: the format's
    usual scale, a scale that is no power of two, and once with normalisation"""
    import torch
    import srsgpu_phy as s
    rng = np.random.default_rng(1000 * fmt + N)
    n, gsz = 3, 14 * 12 * nof_prb
    v = _int_rows(rng, fmt, N, n)
    d_buf, d_tab = _scattered(torch, rng, list(v), [2, 0, 1])
    plain, norm = s.OfdmRx(nof_prb, N), s.OfdmRx(nof_prb, N, normalize=True)
    for o, scale in ((plain, DEFAULT_SCALE[fmt]), (plain, ODD_SCALE), (norm, ODD_SCALE)):
        want = _strided(torch, o, _host_floats(v, scale), gsz)
        got = _from_rows(torch, o, d_tab, n, fmt, scale, gsz)
        assert want.any()
        assert (got == want).all(), (scale, int((got != want).sum()))
    plain.close()
    norm.close()


@pytest.mark.parametrize("nof_prb,N", [(25, 512), (100, 1536)])
def test_sc8_rows_extended_cp(nof_prb, N):
    import torch
    import srsgpu_phy as s
    rng = np.random.default_rng(N + 1)
    n, gsz = 3, 12 * 12 * nof_prb
    v = _int_rows(rng, SC8, N, n, cp=1)
    d_buf, d_tab = _scattered(torch, rng, list(v), [1, 2, 0])
    o = s.OfdmRx(nof_prb, N, cp=1)
    for scale in (DEFAULT_SCALE[SC8], ODD_SCALE):
        want = _strided(torch, o, _host_floats(v, scale), gsz)
        got = _from_rows(torch, o, d_tab, n, SC8, scale, gsz)
        assert want.any() and (got == want).all(), scale
    o.close()


def test_cf32_rows_equal_the_strided_call():
    """complex float through the table: only the row addressing differs from the strided call"""
    import torch
    import srsgpu_phy as s
    nof_prb, N, n = 25, 512, 3
    rng = np.random.default_rng(3)
    gsz = 14 * 12 * nof_prb
    x = (rng.standard_normal((n, 15 * N)) + 1j * rng.standard_normal((n, 15 * N))).astype(np.complex64)
    d_buf, d_tab = _scattered(torch, rng, list(x), [1, 2, 0])
    o = s.OfdmRx(nof_prb, N)
    want = _strided(torch, o, x, gsz)
    got = _from_rows(torch, o, d_tab, n, 0, 0.0, gsz)  # in_scale is ignored
    assert want.any() and (got == want).all()
    o.close()


def test_rows_call_refuses_bad_arguments():
    import torch
    import srsgpu_phy as s
    nof_prb, N = 25, 512
    gsz = 14 * 12 * nof_prb
    o = s.OfdmRx(nof_prb, N)
    d_buf = torch.zeros(15 * N * 2, dtype=torch.int8, device="cuda")
    d_tab = torch.tensor([d_buf.data_ptr()], dtype=torch.int64, device="cuda")
    d_g = torch.zeros(gsz, dtype=torch.complex64, device="cuda")
    assert o.rx_rows_dev(1, d_tab.data_ptr(), 3, 1.0, d_g.data_ptr(), gsz) == -1
    assert o.rx_rows_dev(1, d_tab.data_ptr(), SC8, 1.0, d_g.data_ptr(), gsz - 1) == -1
    assert o.rx_rows_dev(1, None, SC8, 1.0, d_g.data_ptr(), gsz) == -1
    assert o.rx_rows_dev(1, d_tab.data_ptr(), SC8, 1.0, None, gsz) == -1
    assert o.rx_rows_dev(1, d_tab.data_ptr(), SC8, 1.0, d_g.data_ptr(), gsz) == 0
    torch.cuda.synchronize()
    assert not d_g.cpu().numpy().any()  # zeros in, zeros out
    o.close()
