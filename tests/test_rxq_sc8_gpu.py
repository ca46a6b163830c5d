"""8-bit I/Q through the subframe queue (SRSGPU_RXQ_SC8): the same TBs, iterations and noise
estimates, bit for bit, as the staged complex-float path on the same sample values, whether the OFDM
kernel converts the samples in its first load (the default for SC8) or the ingest kernel does first
(SRSGPU_RXQ_FUSE=0), with registered rows DMA'd or read over the bus, and staged or registered rows
in any mix and order.

The case is test_rx_queue_gpu's: 12 subframes, 5 MHz, MCS 28, 30 dB. Quantised to 8 bits with the
peak at 127 such subframes keep an SQNR of at least 38 dB (numpy, 40 draws at N = 128, 512 and 1536), so
beside the 30 dB channel about 29.4 dB are left for a code that needs roughly 19 dB: the reference run
on the dequantised samples must ack every TB with the transmitted bytes before anything is compared."""
import numpy as np
import pytest

from test_rx_queue_gpu import _queue_case, _run_queue

pytestmark = pytest.mark.gpu


def _quantise(xs, dtype, top):
    scale = float(max(np.abs(x.view(np.float32)).max() for x in xs)) / top
    q = [np.round(x.view(np.float32) / scale).astype(dtype).reshape(-1, 2) for x in xs]
    xq = [(v.astype(np.float32) * np.float32(scale)).reshape(-1).view(np.complex64) for v in q]
    return scale, q, xq


@pytest.fixture(scope="module")
def case(oracle):
    """the subframes as int8 and int16 samples, and what today's path (staged complex floats of the same
    values) decodes from each: computed once, read by every test below"""
    import srsgpu_phy as s
    nof_prb, cell_id, tbs, N, xs, datas, sfs = _queue_case(oracle)
    n = len(xs)
    c = dict(nof_prb=nof_prb, cell_id=cell_id, tbs=tbs, N=N, datas=datas, sfs=sfs, n=n)
    c["scale8"], c["sc8"], c["xq8"] = _quantise(xs, np.int8, 127.0)
    c["scale16"], c["sc16"], c["xq16"] = _quantise(xs, np.int16, 32767.0)
    q = s.RxQueue(nof_prb, cell_id, N, nof_softbuffers=n, max_batch=n, max_wait_us=200000)
    c["want"] = _run_queue(s, q, c["xq8"], sfs, nof_prb, tbs)
    c["want16"] = _run_queue(s, q, c["xq16"], sfs, nof_prb, tbs)
    assert q.ingest_stats() == (0, 2 * n)
    q.close()
    return c


def _same(got, want):
    return got[:3] == want[:3] and all((a == b).all() for a, b in zip(got[3], want[3]))


def _queue(s, c, **kw):
    return s.RxQueue(c["nof_prb"], c["cell_id"], c["N"], nof_softbuffers=c["n"], max_batch=c["n"],
                     max_wait_us=200000, **kw)


def _run(s, q, c, rows, sfs=None):
    return _run_queue(s, q, rows, c["sfs"] if sfs is None else sfs, c["nof_prb"], c["tbs"])


def test_reference_runs_decode_the_quantised_subframes(case):
    c = case
    assert np.abs(np.stack(c["sc8"])).max() == 127
    for want in (c["want"], c["want16"]):
        assert all(r == 0 for r in want[0])
        for i in range(c["n"]):
            assert (want[3][i][:c["tbs"] // 8] == c["datas"][i]).all(), i


@pytest.mark.parametrize("ingest", ["dma", "kernel"])
@pytest.mark.parametrize("fuse", [None, "0"])
def test_sc8_ingest(case, fuse, ingest, monkeypatch):
    import torch
    import srsgpu_phy as s
    c, n, want = case, case["n"], case["want"]
    monkeypatch.setenv("SRSGPU_RXQ_INGEST", ingest)
    if fuse is None:
        monkeypatch.delenv("SRSGPU_RXQ_FUSE", raising=False)
    else:
        monkeypatch.setenv("SRSGPU_RXQ_FUSE", fuse)
    q = _queue(s, c)
    q.set_input_format(q.SC8, c["scale8"])
    sc = c["sc8"]
    # staged
    assert _same(_run(s, q, c, sc), want)
    assert q.ingest_stats() == (0, n)
    # every row in a registered block
    blk = np.stack(sc)
    q.register(blk)
    assert _same(_run(s, q, c, list(blk)), want)
    assert q.ingest_stats() == (n, n)
    # out of address order, one row twice in the batch
    perm = [5, 0, 0, 11, 3, 2, 1, 4, 10, 9, 7, 6][:n]
    got = _run(s, q, c, [blk[p] for p in perm], [c["sfs"][p] for p in perm])
    for i, p in enumerate(perm):
        assert (got[0][i], got[1][i], got[2][i]) == (want[0][p], want[1][p], want[2][p]), i
        assert (got[3][i] == want[3][p]).all(), i
    q.unregister(blk)
    # registered and staged rows mixed in one batch
    half = np.stack(sc[::2])
    q.register(half)
    z0, s0 = q.ingest_stats()
    assert _same(_run(s, q, c, [half[i // 2] if i % 2 == 0 else sc[i] for i in range(n)]), want)
    assert q.ingest_stats() == (z0 + (n + 1) // 2, s0 + n // 2)
    q.unregister(half)
    # a registered td pointer 8 bytes past a 16-byte boundary is staged
    raw = np.zeros(sc[0].nbytes + 32, np.uint8)
    q.register(raw)
    off = (8 - raw.ctypes.data) % 16
    mis = raw[off:off + sc[0].nbytes].view(np.int8).reshape(sc[0].shape)
    assert mis.ctypes.data % 16 == 8
    mis[:] = sc[0]
    z0, s0 = q.ingest_stats()
    assert _same(_run(s, q, c, [mis] + sc[1:]), want)
    assert q.ingest_stats() == (z0, s0 + n)
    q.unregister(raw)
    # rows of a registered block with a junk row between every two
    gap = np.empty((2 * n,) + sc[0].shape, np.int8)
    gap[0::2] = blk
    gap[1::2] = np.random.default_rng(5).integers(-128, 128, size=blk.shape, dtype=np.int8)
    q.register(gap)
    assert _same(_run(s, q, c, list(gap[0::2])), want)
    q.unregister(gap)
    q.close()
    torch.cuda.synchronize()


def test_sc16_fused(case, monkeypatch):
    """SRSGPU_RXQ_FUSE=1: int16 rows take the OFDM kernel's load too, staged and registered"""
    import torch
    import srsgpu_phy as s
    c, n = case, case["n"]
    monkeypatch.setenv("SRSGPU_RXQ_FUSE", "1")
    monkeypatch.delenv("SRSGPU_RXQ_INGEST", raising=False)
    q = _queue(s, c)
    q.set_input_format(q.SC16, c["scale16"])
    assert _same(_run(s, q, c, c["sc16"]), c["want16"])
    blk = np.stack(c["sc16"])
    q.register(blk)
    assert _same(_run(s, q, c, list(blk)), c["want16"])
    assert q.ingest_stats() == (n, n)
    q.unregister(blk)
    q.close()
    torch.cuda.synchronize()


def test_format_switching_on_one_queue(case, monkeypatch):
    import torch
    import srsgpu_phy as s
    c = case
    monkeypatch.delenv("SRSGPU_RXQ_FUSE", raising=False)
    monkeypatch.delenv("SRSGPU_RXQ_INGEST", raising=False)
    q = _queue(s, c)
    assert _same(_run(s, q, c, c["xq8"]), c["want"])
    q.set_input_format(q.SC8, c["scale8"])
    assert _same(_run(s, q, c, c["sc8"]), c["want"])
    q.set_input_format(q.SC16, c["scale16"])
    assert _same(_run(s, q, c, c["sc16"]), c["want16"])
    q.set_input_format(q.SC8, c["scale8"])
    assert _same(_run(s, q, c, c["sc8"]), c["want"])
    with pytest.raises(RuntimeError):
        q.set_input_format(3)
    q.close()
    torch.cuda.synchronize()


def test_sc8_default_scale_is_one_128th(case, monkeypatch):
    """scale 0 means 1 / 128: the same grids, so the same TBs, as complex floats of v / 128 (a power of
    two: exact)"""
    import torch
    import srsgpu_phy as s
    c = case
    monkeypatch.delenv("SRSGPU_RXQ_FUSE", raising=False)
    q = _queue(s, c)
    x128 = [(v.astype(np.float32) / np.float32(128.0)).reshape(-1).view(np.complex64) for v in c["sc8"]]
    want = _run(s, q, c, x128)
    q.set_input_format(q.SC8)
    assert _same(_run(s, q, c, c["sc8"]), want)
    assert all(r == 0 for r in want[0])
    q.close()
    torch.cuda.synchronize()


def test_sc8_two_rx_antennas(monkeypatch):
    """a two-antenna cell: the batch's row table holds [subframe][antenna] rows. SISO subframes on 2 rx
    antennas (the traffic generator's), quantised to 8 bits: the SC8 batch, one antenna of every
    subframe registered and the other staged, equals its complex-float twin and acks every TB"""
    import torch
    import srsgpu_phy as s
    import srsgpu_traffic as tr
    monkeypatch.delenv("SRSGPU_RXQ_FUSE", raising=False)
    monkeypatch.delenv("SRSGPU_RXQ_INGEST", raising=False)
    m = tr.MimoSubframes(torch, torch.device("cuda"), 6, seed=29, snr_db=30.0, mimo=s.MIMO_SINGLE_ANTENNA, mcs=20,
                         nof_prb=25, ce_rows=False, nof_ports=1)
    torch.cuda.synchronize()
    x = m.x.cpu().numpy().reshape(m.n * 2, 15 * m.N)
    scale, sc, xq = _quantise(list(x), np.int8, 127.0)
    tx = m.d_data_tx.cpu().numpy().reshape(m.n, 2, m.dlen)
    nb = m.tbs // 8
    q = s.RxQueue(25, m.cell_id, m.N, nof_ports=1, nof_rx_ant=2, nof_softbuffers=m.n, max_batch=m.n,
                  max_wait_us=200000)
    reg = np.stack(sc[0::2])  # antenna 0 of every subframe
    q.register(reg)

    def run(rows):
        outs = [np.zeros(m.dlen, np.uint8) for _ in range(m.n)]
        items = []
        for j, i in enumerate(m.kept):
            sf = s.make_sf(sf_idx=1 + (i % 4), lstart=1, nof_prb=25, mod=3, rnti=1234, tbs=m.tbs, softbuffer=j)
            sf.nof_re = m.pd.nof_re(sf)
            items.append(q.item(rows[j], sf, [outs[j]]))
        tickets = [q.submit(it) for it in items]
        q.flush()
        assert all(q.wait(t) == 0 for t in tickets)
        return [it.ret[0] for it in items], [it.noi[0] for it in items], [it.noise for it in items], outs

    want = run([[xq[2 * j], xq[2 * j + 1]] for j in range(m.n)])
    assert all(r == 0 for r in want[0])
    for j in range(m.n):
        assert (want[3][j][:nb] == tx[j, 0, :nb]).all(), j
    q.set_input_format(q.SC8, scale)
    z0, s0 = q.ingest_stats()
    got = run([[reg[j], sc[2 * j + 1]] for j in range(m.n)])
    assert _same(got, want)
    assert q.ingest_stats() == (z0 + m.n, s0 + m.n)
    q.unregister(reg)
    q.close()
    m.close()
    torch.cuda.synchronize()
