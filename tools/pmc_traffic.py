#!/usr/bin/env python
"""Reduce rocprofv3 PMC passes to HBM bytes per launch per kernel.

    rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d DIR/fetch -o f -- python3 bench.py ...
    rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d DIR/write -o w -- python3 bench.py ...
    python tools/pmc_traffic.py DIR/fetch DIR/write > profiles/rNN_pmc_traffic.json

Corrections (MI355X_MICROARCH.md, HBM section): the counters are in KiB-like units of 1024 B
(hbm_bytes = counter * 1024); on gfx950 FETCH_SIZE tallies 128-B requests at 64 B, i.e. it reads
exactly half of the bytes of a wide coalesced streaming read, so the read side is doubled.
WRITE_SIZE is exact for 16-B-per-lane streaming stores.
"""
import csv
import glob
import json
import os
import sys
from collections import defaultdict


def load(dirname, counter):
    out = defaultdict(lambda: [0, 0.0])
    files = glob.glob(os.path.join(dirname, "**", "*counter_collection.csv"), recursive=True)
    for fn in files:
        with open(fn) as f:
            for row in csv.DictReader(f):
                if row.get("Counter_Name") != counter:
                    continue
                k = row["Kernel_Name"]
                out[k][0] += 1
                out[k][1] += float(row["Counter_Value"])
    return out


def short(name):
    for key in ("gemm_nt_f16x2_cc_kernel", "dft_ct_kernel", "dft_h2_adjmix_kernel", "dft_h2_adjmix_reduce_kernel", "dft_h2_kernel", "dft_rx3_kernel", "dft_fold4_kernel", "dft_fold_kernel", "gemm_f32_kernel<128, 128>", "gemm_f32_kernel<64, 128>", "gemm_f32_kernel<128, 64>",
                "gemm_f32_kernel<64, 64>", "spmm_group_gather_f16_kernel", "spmm_group_scatter_kernel", "spmm_rows_f16_kernel", "spmm_rows_kernel", "specmix_fwd_ilv_kernel", "specmix_adj_ilv_kernel", "specmix_fwd_kernel", "specmix_adj_kernel",
                "fill_zero_kernel", "y_from_cpart_kernel", "ymat_from_y_kernel", "huber_vox_grad_kernel", "huber_vox_curv_kernel", "mmmg_update_kernel"):
        if key in name:
            return key
    return None


def main():
    fetch = load(sys.argv[1], "FETCH_SIZE")
    write = load(sys.argv[2], "WRITE_SIZE")
    res = {}
    for name in set(fetch) | set(write):
        s = short(name)
        if s is None:
            continue
        e = res.setdefault(s, {"launches": 0, "fetch_bytes": 0.0, "write_bytes": 0.0, "symbols": {}})
        # several symbols may share a key (template instances of one kernel): launches add over symbols, and a symbol is
        # seen once in each of the two passes
        n = max(fetch[name][0] if name in fetch else 0, write[name][0] if name in write else 0)
        e["launches"] += n
        f = fetch[name][1] * 1024.0 * 2.0 if name in fetch else 0.0    # gfx950 correction
        w = write[name][1] * 1024.0 if name in write else 0.0
        e["fetch_bytes"] += f
        e["write_bytes"] += w
        e["symbols"][name.split("::")[-1]] = {"launches": n, "fetch_bytes_per_launch": f / max(1, n),
                                              "write_bytes_per_launch": w / max(1, n)}
    for s, e in res.items():
        n = max(1, e["launches"])
        e["hbm_bytes_per_launch"] = (e["fetch_bytes"] + e["write_bytes"]) / n
        e["fetch_bytes_per_launch"] = e["fetch_bytes"] / n
        e["write_bytes_per_launch"] = e["write_bytes"] / n
    json.dump(res, sys.stdout, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
