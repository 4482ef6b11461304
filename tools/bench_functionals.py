"""Cost of cx_linear_moments beside cx_sample_posterior at S = K on the same handle: the median of 20 synchronised
calls after a warm-up, on §4g's three configurations; the functionals are window means of 1,000 consecutive states.

    python tools/bench_functionals.py [--small]

Prints one JSON line per configuration: wall milliseconds of both calls and the bytes of §4i (links read twice, u and g written and
read, K² + K doubles out; the sampler: links once, z written and read, S n d doubles out and copied to the host)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cortex.jl_amd as cx  # noqa: E402
from cortex.jl_amd import _lib as L  # noqa: E402


def median_ms(f, n=20):
    f()
    ts = []
    for _ in range(n):
        t0 = time.perf_counter()
        f()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", action="store_true", help="a hundredth of the sizes (a quick check of the tool itself)")
    a = ap.parse_args()
    q = 100 if a.small else 1
    configs = [("lgssm_chain d=4 (C3)", lambda: cx.synth.lgssm_chain(1_000_000 // q, d=4), L.SCHED_CHAIN_SCAN, 8),
               ("ssm_chain (C2)", lambda: cx.synth.ssm_chain(250_001 // q, seed=1234), L.SCHED_CHAIN_SCAN, 64),
               ("tree_model deep", lambda: cx.synth.tree_model(200_000 // q, shape="deep", observe=0.2), L.SCHED_TREE, 64)]
    for name, make, sched, K in configs:
        model = make()
        d = model.dim
        dev = cx.DeviceGraph(dim=d, schedule=sched)
        cx.synth.load_into_device(model, dev)
        dev.sweep(1)
        x = np.asarray(model.x_ids, np.int64)
        n, w = len(x), min(1000, len(x))
        starts = np.linspace(0, n - w, K).astype(np.int64)
        off = np.arange(K + 1, dtype=np.int64) * w
        ids = np.concatenate([x[s:s + w] for s in starts])
        wt = np.full((K * w, d), 1.0 / w)
        t_fn = median_ms(lambda: dev.linear_moments((off, ids, wt)))
        t_mean = median_ms(lambda: dev.linear_moments((off, ids, wt), cov=False))
        t_sp = median_ms(lambda: dev.sample_posterior(K, seed=1, variable_ids=x))
        _, _, cnt = dev.linear_moments((off, ids, wt))
        npos, link = cnt["free"], (2 * d * d + d) * 8
        fn_bytes = npos * (2 * link + 8 * d * K * 5) + (K * K + K) * 8      # links twice; u: zero, walk read + write, noise read; g: write, read
        sp_bytes = npos * (link + 8 * d * K * 2) + 2 * K * n * d * 8          # links once; z write + read; out written, copied
        print(json.dumps({"config": name, "n": int(n), "dim": d, "K": K, "linear_moments_ms": round(t_fn, 3), "means_only_ms": round(t_mean, 3),
                          "sample_posterior_ms": round(t_sp, 3), "linear_moments_bytes": int(fn_bytes), "sample_posterior_bytes": int(sp_bytes)}), flush=True)
        dev.close()


if __name__ == "__main__":
    main()
