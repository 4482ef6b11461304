"""lab: when every wave of one deep-sweep launch starts and ends (cx_sweep_deep.hip under CX_DEEP_STAMPS).  Needs a stamped library:
  CX_BUILD_DEEP_STAMPS=1 python -m cortex.jl_amd.build --force     (=2: column-edge waves take the general instance, the dispatch before it)
kept aside and named in CORTEX_HIP_LIB; rebuild the shipped library afterwards.  A few warm calls on the flagship grid, then one call of 17
sweeps per depth, whose last deep launch is the one whose records remain.  Per class of wave (interior; column-edge: strips 0 and last of a
row-interior segment; row-edge: top and bottom segment of an interior strip; corner) and per XCD: the count, the median and range of the
wave's duration and of its end after the launch's first start; which classes share a SIMD; the launch's span; who is alive after the median
interior wave has ended.
python tools/lab/deep_sweep_stamps.py [N] [depths, default 4,3]"""
import collections
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import cortex.jl_amd as cx  # noqa: E402
from cortex.jl_amd import _lib as L  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 1415
DEPTHS = [int(x) for x in (sys.argv[2] if len(sys.argv) > 2 else "4,3").split(",")]
MAX_WAVES = 4096
CLASSES = ("interior", "column-edge", "row-edge", "corner")

read = L.load().cx_lab_deep_stamps          # (AttributeError: not a stamped library)
read.restype = C.c_int32
read.argtypes = [C.c_void_p, C.c_int32]
model = cx.synth.gaussian_grid(N, N, seed=1234)


def stamps():
    buf = np.zeros((MAX_WAVES, 8), dtype=np.uint64)
    assert read(buf.ctypes.data, MAX_WAVES) == MAX_WAVES
    return buf[buf[:, 6] != 0]


def line(name, sel, dur, end):
    if not sel.any():
        return f"  {name:12s} {0:5d}"
    d, e = dur[sel], end[sel]
    return (f"  {name:12s} {int(sel.sum()):5d}   duration {np.median(d):7.2f} us ({d.min():7.2f} - {d.max():7.2f})   "
            f"end after first start {np.median(e):7.2f} us ({e.min():7.2f} - {e.max():7.2f})")


for K in DEPTHS:
    os.environ["CX_SWEEP_PAIRS"] = "1"
    os.environ["CX_SWEEP_DEPTH"] = str(K)
    dev = cx.DeviceGraph(schedule=L.SCHED_FUSED)
    cx.synth.load_into_device(model, dev, 1e6)
    for _ in range(3):
        dev.sweep(201)
    dev.sync()
    stamps()                                  # (cleared)
    dev.sweep(17)
    dev.sync()
    rec = stamps()
    st = dev.sweep_deep_stats()
    R, cols = st["rows"], 64 - 2 * (K - 1)
    nseg, nstrips = -(-N // R), -(-N // cols)
    strip, seg = (rec[:, 5] & 0xFFFFFFFF).astype(np.int64), (rec[:, 5] >> 32).astype(np.int64)
    assert len(rec) == nstrips * nseg and len(set(zip(strip.tolist(), seg.tolist()))) == len(rec), (len(rec), nstrips, nseg)
    r0, r1 = seg * R, np.minimum(seg * R + R, N)
    rows_in = (r0 - (K - 1) >= 1) & (r1 + (K - 1) - 1 <= N - 2)
    cols_in = (strip * cols - (K - 1) >= 1) & (strip * cols - (K - 1) + 63 <= N - 2)
    cls = np.where(rows_in, np.where(cols_in, 0, 1), np.where(cols_in, 2, 3))
    inst = rec[:, 6].astype(np.int64) - 1     # 0 general, 1 interior, 2 column-edge
    t_first = rec[:, 0].min()
    dur = (rec[:, 1] - rec[:, 0]).astype(np.float64) / 100.0                      # (the 100 MHz clock)
    end = (rec[:, 1] - t_first).astype(np.float64) / 100.0
    start = (rec[:, 0] - t_first).astype(np.float64) / 100.0
    cyc = (rec[:, 3] - rec[:, 2]).astype(np.float64)
    hw, xcc = rec[:, 4] & 0xFFFFFFFF, (rec[:, 4] >> 32).astype(np.int64)
    simd = ((xcc.astype(np.uint64) << 16) | (((hw >> 8) & 0xFF) << 2) | ((hw >> 4) & 3)).astype(np.int64)      # XCC | SE, SH, CU | SIMD
    print(f"==== depth {K}, {N} x {N}, {R} rows per segment: {len(rec)} working waves ({nstrips} strips x {nseg} segments), instances general / interior / "
          f"column-edge {[(inst == i).sum() for i in range(3)]}; launch span {end.max():.2f} us; shader clock per 100 MHz tick {np.median(cyc / (dur * 100.0)):.2f}; "
          f"starts {np.median(start):.2f} us median, {start.max():.2f} last")
    print("by class:")
    for i, name in enumerate(CLASSES):
        print(line(name, cls == i, dur, end))
    print("shader-clock cycles per wave, median by class: " + ", ".join(f"{name} {np.median(cyc[cls == i]):.0f}" for i, name in enumerate(CLASSES) if (cls == i).any()))
    print("by XCD (all classes, then each class):")
    for x in sorted(set(xcc.tolist())):
        print(line(f"XCD {x}", xcc == x, dur, end))
        for i, name in enumerate(CLASSES):
            if ((xcc == x) & (cls == i)).any():
                print("  " + line(name, (xcc == x) & (cls == i), dur, end))
    per_simd = collections.defaultdict(lambda: [0, 0, 0, 0])
    for s, k in zip(simd.tolist(), cls.tolist()):
        per_simd[s][k] += 1
    print(f"SIMDs with work: {len(per_simd)}; waves per SIMD {collections.Counter(sum(v) for v in per_simd.values()).most_common()}")
    for i, name in enumerate(CLASSES[1:], 1):
        print(f"  {name} waves per SIMD that holds any: {sorted(collections.Counter(v[i] for v in per_simd.values() if v[i]).items())}")
    t_int = np.median(end[cls == 0])
    alive = end > t_int
    late = end > t_int + 0.5 * (end.max() - t_int)
    print(f"the median interior wave ends at {t_int:.2f} us, the span at {end.max():.2f}: the stretch between is {end.max() - t_int:.2f} us = {(end.max() - t_int) / end.max():.3f} of the span")
    print("  alive after the median interior end: " + ", ".join(f"{name} {int((alive & (cls == i)).sum())} of {int((cls == i).sum())}" for i, name in enumerate(CLASSES)))
    print("  alive in the second half of that stretch: " + ", ".join(f"{name} {int((late & (cls == i)).sum())}" for i, name in enumerate(CLASSES)))
    last = np.argsort(end)[-12:][::-1]
    print("  the last 12 waves to end: " + "; ".join(f"{CLASSES[cls[j]]} strip {strip[j]} seg {seg[j]} XCD {xcc[j]} {end[j]:.2f}" for j in last))
    dev.close()
