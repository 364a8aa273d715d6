#!/usr/bin/env python3
"""Device ingest (device.canonicalize_device) against the host path it replaces, same process.

Raw input per scale s: the R-MAT tuples of ghs_rmat_tuples at edgefactor 16 (16 * 2^s raw edges with
the generator's repeats and self-loops), decoded on the device, each tuple's orientation flipped by
a hash of its index, weights = a hash of the index. Timed with a host clock around the call (it ends
in a stream synchronise), warmed up, repeated; median, min and max are reported:
  device  canonicalize_device(n, u, v, w) on the device-resident raw arrays
  host    (--host, s20 / s22; at s24 the host sort takes minutes and is skipped) the raw arrays' D2H
          copy, graph.canonicalize (numpy stable argsort), DeviceEdges.from_host (H2D)
  rmat    generate_rmat at the same tuple count: tuple generation + the keys-only sort + unique, the
          device-side yardstick (the pairs sort moves about 1.5x the bytes of that sort)
Every timed size is checked canonical on the device (ghs_check_canonical); with --host the device
result is compared with the host path's, array by array. `bound` is the time the passes' bytes would
take at the HBM rates of the micro-architecture notes (8.0 TB/s spec, 6.29 TB/s measured copy): a
lower bound from a byte count, not a measurement.

    python tools/ingest_bench.py --scale 20 --host --out profiles/r07/ingest_bench.json
    python tools/ingest_bench.py --scale 22 --host --host-repeats 2 --out profiles/r07/ingest_bench.json
    python tools/ingest_bench.py --scale 24 --out profiles/r07/ingest_bench.json      (merges into the file)

--weights {f32,f64,i64}: the weight-rank pass (device.weight_ranks) on the same raw tuples, with
weights of that dtype (a hash of the index as the dtype's bit pattern, about a quarter of them
repeated values). Timed the same way, same process, same input:
  weight_ranks                 the rank pass alone
  canonicalize_rank_weights    canonicalize_device(..., rank_weights=True): ranks + canonicalisation + gather
  canonicalize_uint32          the uint32 canonicalize_device call on the same tuples (the yardstick)
  host                         (--host, s20 / s22) D2H, graph.canonicalize (np.unique + searchsorted rank
                               map, then the sort), DeviceEdges.from_host; compared array by array

    python tools/ingest_bench.py --scale 22 --weights f64 --host --host-repeats 2 --out profiles/r08/ingest_weights.json
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

EF = 16
HBM_SPEC_TBS = 8.0
HBM_COPY_TBS = 6.29
SORT_DIGIT_BITS = 8  # rocPRIM's radix digit for 64-bit keys (one read + one write of a pair per digit)


def spread(ts):
    return {"median_ms": statistics.median(ts) * 1e3, "min_ms": min(ts) * 1e3, "max_ms": max(ts) * 1e3,
            "repeats": len(ts)}


def timed(fn, warmup, repeats, sync):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(repeats):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        ts.append(time.perf_counter() - t0)
    return ts


def raw_rmat(scale, seed):
    """(u, v, w) int32 device tensors of 16 * 2^scale raw edges (uint32 bit patterns)."""
    import torch

    from distributed_ghs_implementation_amd import _native
    from distributed_ghs_implementation_amd.device import _ptr, _stream
    T = EF << scale
    keys = torch.empty(T, dtype=torch.int64, device="cuda")
    _native.check(_native.load().ghs_rmat_tuples(scale, EF, seed, _ptr(keys), _stream()))
    a = keys >> scale
    b = keys & ((1 << scale) - 1)  # a self-loop's marker decodes to (2^s - 1, 2^s - 1): still a self-loop
    del keys
    M = 0xFFFFFFFF

    def mix32(x):  # common.h mix32 on int64 lanes holding uint32 values
        x = ((x ^ (x >> 16)) * 0x7FEB352D) & M
        x = ((x ^ (x >> 15)) * 0x846CA68B) & M
        return x ^ (x >> 16)

    idx = torch.arange(T, dtype=torch.int64, device="cuda")
    flip = (mix32(idx ^ 0x5BD1E995) & 1).bool()
    w = mix32(idx ^ 0x2545F491)
    del idx
    u = torch.where(flip, b, a).to(torch.int32)
    v = torch.where(flip, a, b).to(torch.int32)
    del a, b, flip
    w = torch.where(w >= (1 << 31), w - (1 << 32), w).to(torch.int32)
    torch.cuda.synchronize()
    return u, v, w


def bytes_per_raw_edge(scale, kept_fraction):
    """HBM bytes each pass moves per raw edge (DESIGN.md "Device ingest")."""
    bits = max(1, scale)
    digits = -(-2 * bits // SORT_DIGIT_BITS)
    return {
        "k_canon_keys": 8 + 12,                       # reads u, v; writes key + raw index
        "sort_histogram": 8,                          # one read of the keys
        "sort_digits": digits * 24,                   # per digit: a (key, index) pair read and written
        "k_canon_count": 8,                           # the sorted keys
        "k_canon_write": 8 + kept_fraction * (4 + 4 + 16),  # keys; per survivor: index, w gather, u/v/w/src
        "digits": digits,
    }


def run_scale(scale, seed, warmup, repeats, host, host_repeats):
    import torch

    from distributed_ghs_implementation_amd import _native, canonicalize
    from distributed_ghs_implementation_amd.device import (DeviceEdges, _ptr, _stream, canonicalize_device,
                                                            generate_rmat)
    assert torch.cuda.is_available(), "ingest_bench needs a GPU (no fallback)"
    n, T = 1 << scale, EF << scale
    u, v, w = raw_rmat(scale, seed)
    sync = torch.cuda.synchronize
    keep = {}

    def dev():
        keep["e"] = canonicalize_device(n, u, v, w)
    t_dev = timed(dev, warmup, repeats, sync)
    e = keep["e"]
    ok = ctypes.c_int(0)
    _native.check(_native.load().ghs_check_canonical(n, e.m, _ptr(e.u), _ptr(e.v), _stream(), ctypes.byref(ok)))
    assert ok.value == 1, "the device result is not canonical"
    print(f"s{scale}: device {statistics.median(t_dev) * 1e3:.3f} ms, m = {e.m} of {T}", file=sys.stderr, flush=True)

    def gen():
        keep["g"] = generate_rmat(scale, EF, seed=seed)
    t_gen = timed(gen, 1, repeats, sync)
    keep.pop("g")
    bpe = bytes_per_raw_edge(scale, e.m / T)
    total_b = sum(x for k, x in bpe.items() if k != "digits") * T
    rec = {
        "workload": f"rmat-s{scale}-ef{EF}-raw", "n": n, "m_raw": T, "m": e.m, "seed": seed,
        "temp_bytes": int(_native.load().ghs_canonicalize_temp_bytes(n, T)),
        "device": spread(t_dev), "canonical": True,
        "rmat_generate": spread(t_gen),
        "bytes_per_raw_edge": bpe,
        "bound": {"bytes": total_b, "ms_at_spec_8.0TBs": total_b / (HBM_SPEC_TBS * 1e12) * 1e3,
                  "ms_at_copy_6.29TBs": total_b / (HBM_COPY_TBS * 1e12) * 1e3,
                  "note": "bytes / HBM rate: a lower bound, not a measurement"},
        "host": None,
    }
    if host:
        def host_path():
            hu, hv, hw = (t.cpu().numpy().view("uint32") for t in (u, v, w))
            t1 = time.perf_counter()
            g = canonicalize(n, u=hu, v=hv, w=hw)
            t2 = time.perf_counter()
            keep["h"] = DeviceEdges.from_host(g)
            keep["sort_s"] = t2 - t1
            print(f"s{scale}: host canonicalize {t2 - t1:.2f} s", file=sys.stderr, flush=True)
        t_host = timed(host_path, 0, host_repeats, sync)
        h = keep["h"]
        equal = bool(h.m == e.m and all(torch.equal(a, b) for a, b in zip((e.u, e.v, e.w), (h.u, h.v, h.w))))
        assert equal, "device and host canonical lists differ"
        rec["host"] = dict(spread(t_host), equal_to_device=equal, last_canonicalize_s=keep["sort_s"])
        rec["ratio_host_over_device"] = statistics.median(t_host) / statistics.median(t_dev)
        rec["ratio_host_over_device_worst"] = min(t_host) / max(t_dev)
    else:
        rec["host_note"] = "not measured: the host sort at this size takes minutes"
    return rec


W_DTYPES = {"f32": "float32", "f64": "float64", "i64": "int64"}


def raw_weights(kind, T):
    """T weights of the chosen dtype on the device: a hash of the index mapped into the dtype (both
    signs, far outside [0, 2^32) for i64), about a quarter of them repeated values (index i with
    i % 4 == 0 takes the value of index i // 64 * 64: runs of 16 equal weights spread over the list)."""
    import torch
    M = 0xFFFFFFFF

    def mix32(x):
        x = ((x ^ (x >> 16)) * 0x7FEB352D) & M
        x = ((x ^ (x >> 15)) * 0x846CA68B) & M
        return x ^ (x >> 16)

    idx = torch.arange(T, dtype=torch.int64, device="cuda")
    idx = torch.where(idx % 4 == 0, idx // 64 * 64, idx)
    lo, hi = mix32(idx ^ 0x2545F491), mix32(idx ^ 0x68E31DA4)
    del idx
    # the hash as the dtype's bit pattern: every sign, exponent (denormals too) and mantissa bit in
    # play; an all-ones exponent (inf / NaN) gets its top exponent bit cleared
    if kind == "f32":
        lo = torch.where((lo & 0x7F800000) == 0x7F800000, lo & ~0x40000000, lo)
        w = torch.where(lo >= (1 << 31), lo - (1 << 32), lo).to(torch.int32).view(torch.float32)
    else:
        w = ((hi - (1 << 31)) << 32) | lo
        if kind == "f64":
            e = 0x7FF0000000000000
            w = torch.where((w & e) == e, w & ~(1 << 62), w).view(torch.float64)
    del lo, hi
    torch.cuda.synchronize()
    return w


def weight_bytes_per_edge(kind):
    """HBM bytes per weight of the rank pass (DESIGN.md "Weight ranks on the device")."""
    kb = 4 if kind == "f32" else 8
    digits = 8 * kb // SORT_DIGIT_BITS
    return {
        "k_weight_keys": kb + kb + 4,       # reads the weight; writes key + index
        "sort_histogram": kb,               # one read of the keys
        "sort_digits": digits * 2 * (kb + 4),  # per digit: a (key, index) pair read and written
        "k_rank_count": kb,                 # the sorted keys
        "k_rank_write": kb + 4 + 4,         # keys, indices; a 4-byte scatter per element
        "digits": digits,
    }


def run_weights(scale, seed, warmup, repeats, host, host_repeats, kind):
    """The rank pass on `kind` weights against the uint32 canonicalize_device call on the same raw
    tuples (and, with --host, against graph.canonicalize's host rank map + sort)."""
    import numpy as np
    import torch

    from distributed_ghs_implementation_amd import canonicalize
    from distributed_ghs_implementation_amd.device import DeviceEdges, canonicalize_device, weight_ranks
    assert torch.cuda.is_available(), "ingest_bench needs a GPU (no fallback)"
    n, T = 1 << scale, EF << scale
    u, v, w32 = raw_rmat(scale, seed)
    w = raw_weights(kind, T)
    sync = torch.cuda.synchronize
    keep = {}

    def ranks():
        keep["r"] = weight_ranks(w)
    t_rank = timed(ranks, warmup, repeats, sync)
    distinct = keep.pop("r")[1]

    def whole():
        keep["e"] = canonicalize_device(n, u, v, w, rank_weights=True)
    t_whole = timed(whole, warmup, repeats, sync)
    e = keep["e"]

    def u32():
        keep["c"] = canonicalize_device(n, u, v, w32)
    t_u32 = timed(u32, warmup, repeats, sync)
    assert keep.pop("c").m == e.m
    med = statistics.median
    print(f"s{scale} {kind}: weight_ranks {med(t_rank) * 1e3:.3f} ms, ranked canonicalize {med(t_whole) * 1e3:.3f} ms, "
          f"uint32 canonicalize {med(t_u32) * 1e3:.3f} ms, distinct = {distinct} of {T}", file=sys.stderr, flush=True)
    bpe = weight_bytes_per_edge(kind)
    total_b = sum(x for k, x in bpe.items() if k != "digits") * T
    rec = {
        "workload": f"rmat-s{scale}-ef{EF}-raw", "weights": W_DTYPES[kind], "n": n, "m_raw": T, "m": e.m, "seed": seed,
        "distinct": distinct, "repeated_fraction": 1.0 - distinct / T,
        "weight_ranks": spread(t_rank), "canonicalize_rank_weights": spread(t_whole),
        "canonicalize_uint32": spread(t_u32),
        "ratio_ranks_over_uint32_canonicalize": med(t_rank) / med(t_u32),
        "ratio_ranked_over_uint32_canonicalize": med(t_whole) / med(t_u32),
        "bytes_per_weight": bpe,
        "bound": {"bytes": total_b, "ms_at_spec_8.0TBs": total_b / (HBM_SPEC_TBS * 1e12) * 1e3,
                  "ms_at_copy_6.29TBs": total_b / (HBM_COPY_TBS * 1e12) * 1e3,
                  "note": "bytes / HBM rate: a lower bound, not a measurement"},
        "host": None,
    }
    if host:
        def host_path():
            hu, hv = (t.cpu().numpy().view("uint32") for t in (u, v))
            hw = w.cpu().numpy()
            t1 = time.perf_counter()
            g = canonicalize(n, u=hu, v=hv, w=hw)
            t2 = time.perf_counter()
            keep["h"], keep["g"] = DeviceEdges.from_host(g), g
            keep["sort_s"] = t2 - t1
            print(f"s{scale} {kind}: host canonicalize {t2 - t1:.2f} s", file=sys.stderr, flush=True)
        t_host = timed(host_path, 0, host_repeats, sync)
        h, g = keep["h"], keep["g"]
        equal = bool(h.m == e.m and all(torch.equal(a, b) for a, b in zip((e.u, e.v, e.w), (h.u, h.v, h.w)))
                     and np.array_equal(e.weights.cpu().numpy(), g.weights))
        assert equal, "device and host rank-mapped canonical lists differ"
        rec["host"] = dict(spread(t_host), equal_to_device=equal, last_canonicalize_s=keep["sort_s"])
        rec["ratio_host_over_device"] = med(t_host) / med(t_whole)
        rec["ratio_host_over_device_worst"] = min(t_host) / max(t_whole)
    else:
        rec["host_note"] = "not measured (--host, at s20 / s22)"
    return rec


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--scale", type=int, required=True)
    ap.add_argument("--weights", choices=sorted(W_DTYPES), default=None,
                    help="time the weight-rank pass on float32 / float64 / int64 weights instead")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--host", action="store_true", help="also time D2H + graph.canonicalize + from_host")
    ap.add_argument("--host-repeats", type=int, default=3)
    ap.add_argument("--out", type=str, default=None, help="JSON file to merge the scale into")
    args = ap.parse_args(argv)
    if args.weights:
        rec = run_weights(args.scale, args.seed, args.warmup, args.repeats, args.host, args.host_repeats, args.weights)
    else:
        rec = run_scale(args.scale, args.seed, args.warmup, args.repeats, args.host, args.host_repeats)
    print(json.dumps(rec))
    if args.out:
        doc = {}
        if os.path.exists(args.out):
            with open(args.out) as f:
                doc = json.load(f)
        doc[f"s{args.scale}-{args.weights}" if args.weights else f"s{args.scale}"] = rec
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=2, sort_keys=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
