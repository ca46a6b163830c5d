"""k_win_spread with a partial last chunk: every windowed block size (K / nb > 40, not only the
multiples of 16) on the latency kernel, against k_win_bidir on the same job (decisions and decoder
state bit for bit, SRSGPU_SPREAD=0 selecting k_win_bidir), against the CPU oracle, and through the
drop-in srslte_tdec_iteration / _8bit protocol whose launch also writes the decision bytes.

The shapes are the smallest that reach each way the partial chunk can go wrong: L = K / nb odd or
= 2 mod 4 (the alpha prepass leaves the T4 groups), n = L mod 16 of 1, 2, 3 and 15, the smallest
admitted L = 41, K no multiple of 32 (the byte rows end inside a word), an empty half pair, and the
headline K = 5824 with 7 and 16 pairs."""
import os

import numpy as np
import pytest

from srsgpu_testlib import AUTO, AVX_WINDOW, SSE_WINDOW, make_cb, make_cb8, natural_to_sb

pytestmark = pytest.mark.gpu

AUTO8 = 16  # SRSGPU_TDEC_AUTO_8BIT


@pytest.fixture(scope="module")
def s():
    import srsgpu_phy
    return srsgpu_phy


def _run(s, impl, sb, ins, K, nh, spread):
    os.environ["SRSGPU_SPREAD"] = "1" if spread else "0"
    s.knobs_reload()
    b = s.TdecBatch(len(ins), 6144)
    try:
        s.prof_reset()
        s.prof_enable(True)
        out = b.run(impl, sb, ins, K, nh)
        s.prof_enable(False)
        used = s.prof_get("k_win_spread")[1]
        st = None if impl == s.SRSGPU_TDEC_AUTO_8BIT else [b.read_state(i, K) for i in range(len(ins))]
    finally:
        b.close()
        os.environ.pop("SRSGPU_SPREAD", None)
        s.knobs_reload()
    return out, st, used


@pytest.mark.parametrize("impl,K,sb,n", [
    (AUTO, 816, 0, 1),         # nb 16, L = 51: odd, n = 3, nc = 4; one block, half the pair empty
    (AUTO, 1008, 1, 3),        # L = 63, n = 15; odd block count
    (AUTO, 1056, 0, 2),        # L = 66 = 2 mod 4, n = 2
    (AUTO, 5824, 0, 13),       # L = 364, n = 12: the C3 transport block's 7 pairs
    (AUTO, 5824, 1, 32),       # 16 pairs
    (AVX_WINDOW, 656, 0, 1),   # manual, L = 41: the smallest admitted, nc = 3, n = 9
    (AVX_WINDOW, 784, 0, 2),   # L = 49, n = 1
    (SSE_WINDOW, 408, 0, 1),   # nb 8, DIV = 1, L = 51; K no multiple of 32
    (SSE_WINDOW, 504, 0, 5),   # L = 63
    (SSE_WINDOW, 800, 0, 2),   # L = 100, n = 4
    (AUTO8, 2112, 0, 1),       # nb 32, L = 66
    (AUTO8, 5824, 1, 3),       # L = 182, n = 6
    (AUTO8, 816, 0, 4),        # 8-bit nb 16, L = 51
    (AUTO8, 6080, 0, 2)])      # L = 190, n = 14
def test_partial_equals_bidir(s, oracle, impl, K, sb, n):
    assert s.SRSGPU_TDEC_AUTO_8BIT == AUTO8
    rng = np.random.default_rng(K * 7 + n + sb)
    ins = []
    for i in range(n):
        if impl == s.SRSGPU_TDEC_AUTO_8BIT:
            _, llr = make_cb8(K, float(rng.choice([1.0, 3.0])), 77 * K + i, float(rng.choice([8.0, 64.0])), oracle)
            nsb = oracle.lib.orc_autoimp_subblocks_8bit(K)
            x = natural_to_sb(llr, K, nsb) if (sb and nsb >= 16) else llr
        else:
            _, llr = make_cb(K, float(rng.uniform(0.5, 3.0)), int(rng.integers(1 << 30)), oracle)
            nsb = oracle.lib.orc_autoimp_subblocks(K)
            x = natural_to_sb(llr, K, nsb) if (sb and impl == AUTO and nsb) else llr
        ins.append(x.astype(np.int16))
    if impl == AUTO and n == 1:  # full-range inputs: every saturating corner
        x = rng.integers(-32768, 32768, ins[0].size).astype(np.int16)
        ins = [x]
    counts = (1, 2, 3, 5)
    orc = None
    if impl != s.SRSGPU_TDEC_AUTO_8BIT and not sb:  # 16-bit, natural layout: the oracle's decisions too
        orc = [oracle.tdec_run(impl, 0, x, K, max(counts))[0] for x in ins]
    for nh in counts:
        got, st, used = _run(s, impl, sb, ins, K, nh, True)
        ref, rst, used0 = _run(s, impl, sb, ins, K, nh, False)
        assert used == nh and used0 == 0, (used, used0)
        np.testing.assert_array_equal(got, ref, err_msg="impl=%d K=%d nh=%d" % (impl, K, nh))
        if st is not None:
            for i in range(n):
                assert (st[i][0] == rst[i][0]).all() and (st[i][1] == rst[i][1]).all(), (impl, K, nh, i)
        if orc is not None:
            for i in range(n):
                np.testing.assert_array_equal(got[i], orc[i][nh - 1], err_msg="oracle impl=%d K=%d nh=%d cb=%d"
                                              % (impl, K, nh, i))


def _knobs(s, poll):
    os.environ["SRSGPU_SPREAD"], os.environ["SRSGPU_SPREAD_POLL"] = "1", poll
    s.knobs_reload()


def _knobs_restore(s):
    os.environ.pop("SRSGPU_SPREAD", None)
    os.environ.pop("SRSGPU_SPREAD_POLL", None)
    s.knobs_reload()


@pytest.mark.parametrize("poll", ["1", "0"])
def test_partial_dropin(s, oracle, poll):
    """one srslte_tdec_iteration call per half-iteration on one handle, block sizes with and without
    a partial chunk in a row: every call is one k_win_spread launch that writes the bytes (no
    k_decide), equal to the oracle's decisions after every half-iteration"""
    _knobs(s, poll)
    try:
        d = s.Tdec(6144)
        d.force_not_sb()
        s.prof_reset()
        s.prof_enable(True)
        for i, K in enumerate((5824, 816, 408, 1008, 6144, 5824)):
            _, llr = make_cb(K, 1.0 + 0.3 * i, 5151 + i, oracle)
            ref = oracle.tdec_run(AUTO, 0, llr, K, 8)[0]
            assert d.new_cb(K) == 0
            out = np.zeros(K // 8, np.uint8)
            for h in range(8):
                d.iteration(llr, out)
                assert (out == ref[h]).all(), (poll, K, h)
        s.prof_enable(False)
        assert s.prof_get("k_win_spread")[1] == 48 and s.prof_get("k_decide")[1] == 0
        d.free()
    finally:
        s.prof_enable(False)
        _knobs_restore(s)


@pytest.mark.parametrize("poll", ["1", "0"])
def test_partial_dropin_8bit(s, oracle, poll):
    """the same through srslte_tdec_iteration_8bit (8-bit AUTO: 32 sub-blocks, L = 66 and 182)"""
    _knobs(s, poll)
    try:
        d = s.Tdec(6144)
        d.force_not_sb()
        s.prof_reset()
        s.prof_enable(True)
        for i, K in enumerate((2112, 5824)):
            _, llr = make_cb8(K, 4.0 + i, 6161 + i, 20.0, oracle)
            ref = oracle.tdec8_run(AUTO, 0, llr, K, 8)
            assert ref is not None
            buf = np.zeros(3 * (6144 + 32) + 64, np.int8)
            buf[:llr.size] = llr
            assert d.new_cb(K) == 0
            out = np.zeros(K // 8, np.uint8)
            for h in range(8):
                d.iteration_8bit(buf, out)
                assert (out == ref[h]).all(), (poll, K, h)
        s.prof_enable(False)
        assert s.prof_get("k_win_spread")[1] == 16 and s.prof_get("k_decide")[1] == 0
        d.free()
    finally:
        s.prof_enable(False)
        _knobs_restore(s)


def test_partial_run_all(s, oracle):
    """srslte_tdec_run_all / _8bit (all half-iterations in one call) on sizes with a partial chunk:
    one k_win_spread launch per half-iteration, the oracle's last decisions"""
    _knobs(s, "1")
    try:
        d = s.Tdec(6144)
        d.force_not_sb()
        s.prof_reset()
        s.prof_enable(True)
        K = 5824
        _, llr = make_cb(K, 1.2, 8181, oracle)
        out = np.zeros(K // 8, np.uint8)
        assert d.run_all(llr, out, 8, K) == 0
        s.prof_enable(False)
        assert (out == oracle.tdec_run(AUTO, 0, llr, K, 8)[0][-1]).all()
        assert s.prof_get("k_win_spread")[1] == 8
        s.prof_reset()
        s.prof_enable(True)
        K = 2112
        _, llr8 = make_cb8(K, 4.0, 8282, 20.0, oracle)
        buf = np.zeros(3 * (6144 + 32) + 64, np.int8)
        buf[:llr8.size] = llr8
        out = np.zeros(K // 8, np.uint8)
        assert d.run_all_8bit(buf, out, 6, K) == 0
        s.prof_enable(False)
        assert (out == oracle.tdec8_run(AUTO, 0, llr8, K, 6)[-1]).all()
        assert s.prof_get("k_win_spread")[1] == 6
        d.free()
    finally:
        s.prof_enable(False)
        _knobs_restore(s)


@pytest.mark.parametrize("max_cb", [6144, 408])
def test_partial_dropin_row_length(s, oracle, max_cb):
    """K = 408 is no multiple of 32: the 51 decision bytes are right, the byte after them in the
    caller's buffer is untouched, and (handle sized for K = 408: the completion word sits 13 bytes
    after the row) the call still completes through its completion word"""
    K = 408
    _knobs(s, "1")
    try:
        d = s.Tdec(max_cb)
        d.force_not_sb()
        _, llr = make_cb(K, 1.5, 7171, oracle)
        ref = oracle.tdec_run(AUTO, 0, llr, K, 4)[0]
        assert d.new_cb(K) == 0
        out = np.full(K // 8 + 1, 0xA5, np.uint8)
        for h in range(4):
            d.iteration(llr, out)
            assert (out[:K // 8] == ref[h]).all(), h
            assert out[K // 8] == 0xA5
        d.free()
    finally:
        _knobs_restore(s)
