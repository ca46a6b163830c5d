"""bench.py --dump-outputs: the arrays of the last timed step (per TB return code, nof_iterations,
decoded bytes) as float32 .npy files, bounded in size by a fixed sample of the TBs. CPU only: the
receive objects are stand-ins that hold the same attributes as srsgpu_traffic.MixedCells."""
import os
import sys
import types

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def _lane(ntb, nbytes, seed):
    import torch
    rng = np.random.default_rng(seed)
    stride = nbytes + 8
    data = rng.integers(0, 256, ntb * stride, dtype=np.uint8)
    tbs = [{"tbs": 8 * nbytes, "data_offset": i * stride} for i in range(ntb)]
    m = types.SimpleNamespace(tb_list=tbs, d_data=torch.from_numpy(data),
                              d_ret=torch.from_numpy(rng.integers(-1, 1, ntb).astype(np.int32)),
                              d_noi=torch.from_numpy(rng.integers(1, 5, ntb).astype(np.int32)))
    return m, data.reshape(ntb, stride)[:, :nbytes]


def test_outputs_whole_and_in_lane_order(tmp_path):
    import bench
    (m0, d0), (m1, d1) = _lane(5, 33, 1), _lane(3, 33, 2)
    out = bench.tb_outputs([m0, m1])
    assert all(a.dtype == np.float32 for a in out.values())
    assert np.array_equal(out["tb_index"], np.arange(8))
    assert np.array_equal(out["tb_bytes"], np.concatenate([d0, d1]).reshape(-1))
    assert np.array_equal(out["tb_ret"], np.concatenate([m0.d_ret.numpy(), m1.d_ret.numpy()]))
    assert np.array_equal(out["tb_nof_iterations"], np.concatenate([m0.d_noi.numpy(), m1.d_noi.numpy()]))
    bench.write_outputs(str(tmp_path / "d"), out, 0, 1)
    assert sorted(os.listdir(tmp_path / "d")) == ["tb_bytes.npy", "tb_index.npy", "tb_nof_iterations.npy",
                                                  "tb_ret.npy"]
    assert np.array_equal(np.load(tmp_path / "d" / "tb_bytes.npy"), out["tb_bytes"])
    bench.write_outputs(str(tmp_path / "e"), out, 1, 2)
    assert "tb_ret_rank1.npy" in os.listdir(tmp_path / "e")


def test_outputs_sampled_under_the_limit(monkeypatch):
    import bench
    m, d = _lane(64, 100, 3)
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 4 * (3 * 64 + 1050))  # room for 10 TBs' bytes
    a, b = bench.tb_outputs([m]), bench.tb_outputs([m])
    idx = a["tb_index"].astype(int)
    assert idx.size == 10 and np.all(np.diff(idx) > 0)
    assert np.array_equal(a["tb_index"], b["tb_index"])  # the same sample every run
    assert np.array_equal(a["tb_bytes"], d[idx].reshape(-1))
    assert a["tb_ret"].size == 64 and a["tb_nof_iterations"].size == 64
    assert sum(v.nbytes for v in a.values()) <= bench.DUMP_LIMIT_BYTES
