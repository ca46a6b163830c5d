"""Saturated ingest of the subframe queue per sample format and conversion path
(python3 tools/rxq_format_probe.py OUT.json [REPEATS [NSF [BATCH]]]): 20 MHz subframes (100 PRB, MCS 28,
20 dB) at N = 2048 and N = 1536, samples in queue-owned registered memory, DMA ingest, NSF (4096)
subframes through one queue at max_batch BATCH (1024) per run. In one process, alternating (the order
rotates from repeat to repeat), REPEATS (3) times each:

  sc16        int16 I/Q, converted by the ingest kernel (SRSGPU_RXQ_FUSE=0): the baseline
  sc16_fused  int16 I/Q, converted in the OFDM kernel's first load (SRSGPU_RXQ_FUSE=1)
  sc8         int8 I/Q, converted by the ingest kernel (SRSGPU_RXQ_FUSE=0)
  sc8_fused   int8 I/Q, converted in the OFDM kernel's first load (SRSGPU_RXQ_FUSE=1)

Writes per size and configuration every run's subframes/s and ingest GB/s (sample bytes handed over /
wall time), their median and spread (max - min over the repeats), and each configuration's median rate
against the baseline's.

For kernel times run it once under rocprofv3 --kernel-trace --stats (no counters in the same run), then
  python3 tools/rxq_format_probe.py --kernel-times <..._kernel_trace.csv> OUT.json [BATCH]
gives, per size, the time per full batch of k_ofdm_rx_c by input format (its template's last argument:
0 complex float out of the ingest kernel, 1 int16, 2 int8) and of k_ingest by the format it converts
(the runs alternate, so an ingest launch belongs to the configuration whose fused twin runs next)."""
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "empower-srslte_amd"))

CONFIGS = (("sc16", "sc16", "0"), ("sc16_fused", "sc16", "1"), ("sc8", "sc8", "0"), ("sc8_fused", "sc8", "1"))
SAMPLE_BYTES = {"sc16": 4, "sc8": 2}


def kernel_times(trace, out_path, B):
    """median us per launch over the launches of full batches (B subframes: 14 B symbols)"""
    import csv
    import re
    rows = sorted(csv.DictReader(open(trace)), key=lambda r: int(r["Start_Timestamp"]))
    ev = []  # (kind, N, format, us) in time order; N and format None for k_ingest until resolved
    for r in rows:
        name, us = r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
        m = re.search(r"k_ofdm_rx_c<(\d+), (?:true|false), (\d)>", name)
        if m:
            N = int(m.group(1))
            spw = 1 if N >= 1024 else 2 if N >= 512 else 4 if N >= 256 else 8
            if int(r["Grid_Size_X"]) in (14 * B // spw, 14 * B // spw * 256):  # workgroups or threads
                ev.append(["ofdm", N, int(m.group(2)), us])
        elif "k_ingest" in name and int(r["Grid_Size_Y"]) == B:
            ev.append(["ingest", None, None, us])
    # an ingest launch feeds the next k_ofdm_rx_c<N, , 0>; its format is the next fused launch's
    nxt_n = nxt_f = None
    for e in reversed(ev):
        if e[0] == "ofdm":
            nxt_n = e[1]
            if e[2]:
                nxt_f = e[2]
        else:
            e[1], e[2] = nxt_n, nxt_f
    out = {}
    for kind, N, f, us in ev:
        if N is None or f is None:
            continue
        key = ("k_ofdm_rx_c input " if kind == "ofdm" else "k_ingest of ") + ("cf32", "sc16", "sc8")[f]
        out.setdefault(str(N), {}).setdefault(key, []).append(us)
    for N in out:
        for key, v in out[N].items():
            out[N][key] = {"launches": len(v), "us_median": round(float(np.median(v)), 1),
                           "us_min": round(min(v), 1), "us_max": round(max(v), 1)}
            print(N, key, out[N][key], flush=True)
    json.dump({"batch": B, "us_per_launch_of_a_full_batch": out}, open(out_path, "w"), indent=1)


def main():
    if sys.argv[1] == "--kernel-times":
        return kernel_times(sys.argv[2], sys.argv[3], int(sys.argv[4]) if len(sys.argv) > 4 else 1024)
    import torch
    import srsgpu_phy as s
    import srsgpu_traffic as tr
    import bench
    out_path = sys.argv[1]
    repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    nsf = int(sys.argv[3]) if len(sys.argv) > 3 else 4096
    B = int(sys.argv[4]) if len(sys.argv) > 4 else 1024
    # 8 B softbuffers and outputs (an item is reused 8 B submissions later): with 4 B, exactly what three
    # batches in flight and one filling hold, the producers wait for a completion before every batch, the
    # 2 ms deadline closes batches a fifth full, and the rate stays at 100 K subframes/s from there on,
    # for every format alike
    snr_db, producers, max_wait_us, live = 20.0, 8, 2000, 8 * B
    dev = torch.device("cuda:0")
    table = json.load(open(os.path.join(REPO, "tests", "golden", "c5_traffic.json")))
    q_cpus = bench.quiet_cpus(3)[0]
    os.environ.pop("SRSGPU_RXQ_INGEST", None)  # DMA ingest
    out = {"workload": "c3_coded_queue_20MHz_64QAM_tbs%d" % bench.C3_TBS, "snr_db": snr_db, "batch": B,
           "subframes_per_run": nsf, "repeats": repeats, "producers": producers, "max_wait_us": max_wait_us, "items_live": live,
           "ingest": "dma",
           "host_memory": "queue-owned (srsgpu_rxq_alloc_host)", "baseline": "sc16", "sizes": {}}
    for fft in (2048, 1536):
        m = tr.MixedCells(table, 1024, torch, dev, seed=22, snr_db=snr_db, prbs=(100,), mcs=28, full_band=True,
                          standard_rate=(fft == 2048))
        c = m.cells[0]
        assert c["N"] == fft, (c["N"], fft)
        x = c["x"].cpu().numpy().reshape(c["n"], 15 * fft).view(np.float32)
        sfs, n_src = c["sfs"], c["n"]
        m.close()
        torch.cuda.synchronize()
        peak = float(np.abs(x).max())
        src = {"sc16": (np.round(x / (peak / 32000.0)).astype(np.int16), peak / 32000.0),
               "sc8": (np.round(x / (peak / 127.0)).astype(np.int8), peak / 127.0)}
        runs = {name: [] for name, _, _ in CONFIGS}
        for rep in range(repeats):
            order = CONFIGS[rep % 4:] + CONFIGS[:rep % 4]  # no configuration always behind the same one
            for name, fmt, fuse in order:
                print("rxq_format_probe: N %d %s run %d" % (fft, name, rep), file=sys.stderr, flush=True)
                os.environ["SRSGPU_RXQ_FUSE"] = fuse  # read when the queue is created
                try:
                    q = s.RxQueue(bench.C3_PRB, 1, fft, nof_softbuffers=live, max_batch=B, max_wait_us=max_wait_us)
                finally:
                    os.environ.pop("SRSGPU_RXQ_FUSE", None)
                q.set_affinity(q_cpus)
                xs, scale = src[fmt]
                q.set_input_format(q.SC8 if fmt == "sc8" else q.SC16, scale)
                ring = q.alloc_host(xs.shape, xs.dtype)
                ring[...] = xs
                dl = (bench.C3_TBS // 8 + 6 + 63) // 64 * 64
                block = q.alloc_host((live, dl), np.uint8)
                count = max(nsf, B)
                items = []
                for i in range(count):
                    sf = sfs[i % n_src]
                    sf.softbuffer[0] = i % live
                    items.append(q.item([ring[i % n_src]], sf, [block[i % live, :bench.C3_TBS // 8 + 6]]))
                warm = [q.submit(items[i]) for i in range(min(B, count))]
                q.flush()
                assert all(q.wait(t) == 0 for t in warm)
                nb0, done0 = q.stats()
                t0 = time.perf_counter()
                t_sub, t_done, status = q.drive(items, producers, reuse=live)
                el = time.perf_counter() - t0
                nb, done = q.stats()
                nb, done = nb - nb0, done - done0
                tmg = q.timing()
                last = items[-min(count, live):]
                runs[name].append({
                    "subframes_per_s": round(count / el, 1),
                    "ingest_GBps": round(count * SAMPLE_BYTES[fmt] * 15 * fft / el / 1e9, 2),
                    "mean_batch": round(done / max(nb, 1), 1), "failed": int((status != 0).sum()),
                    "acked_of_last": "%d/%d" % (sum(1 for it in last if it.ret[0] == 0), len(last)),
                    "dispatcher_us_per_sf": {k: round(v / max(done0 + done, 1) * 1e6, 3) for k, v in tmg.items()}})
                del items, block, ring, last  # views of the queue's blocks: gone before the queue frees them
                q.close()
                torch.cuda.synchronize()
        rec = {}
        for name, fmt, fuse in CONFIGS:
            r = np.array([v["subframes_per_s"] for v in runs[name]])
            g = np.array([v["ingest_GBps"] for v in runs[name]])
            rec[name] = {"format": fmt, "SRSGPU_RXQ_FUSE": fuse, "sample_bytes_per_subframe": SAMPLE_BYTES[fmt] * 15 * fft,
                         "subframes_per_s_median": round(float(np.median(r)), 1),
                         "subframes_per_s_spread": round(float(r.max() - r.min()), 1),
                         "ingest_GBps_median": round(float(np.median(g)), 2),
                         "ingest_GBps_spread": round(float(g.max() - g.min()), 2), "runs": runs[name]}
        base = rec["sc16"]["subframes_per_s_median"]
        for name in rec:
            rec[name]["rate_vs_baseline"] = round(rec[name]["subframes_per_s_median"] / base, 3)
        out["sizes"][str(fft)] = rec
        for name, v in rec.items():
            print(fft, name, v["subframes_per_s_median"], "+-", v["subframes_per_s_spread"], "sf/s",
                  v["ingest_GBps_median"], "GB/s", v["rate_vs_baseline"], flush=True)
    json.dump(out, open(out_path, "w"), indent=1)


if __name__ == "__main__":
    main()
