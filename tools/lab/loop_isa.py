#!/usr/bin/env python3
"""lab: the main loops of the kernels in a hipcc -S listing (`hipcc --offload-arch=gfx950 -O3 -S --cuda-device-only`): for every
outermost loop of a kernel that loads from global memory, its instruction mix and, with -l, its loads and waits in program order.
python tools/lab/loop_isa.py listing.s [kernel name part] [-l]"""
import collections
import re
import sys

args = [a for a in sys.argv[1:] if a != "-l"]
listing = "-l" in sys.argv
txt = open(args[0]).read()
part = args[1] if len(args) > 1 else ""
for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end", txt, re.S | re.M):
    name, body = m.group(1), m.group(2)
    if part not in name:
        continue
    lines = [l.split(";")[0].strip() for l in body.split("\n")]
    lines = [l for l in lines if l and (l.endswith(":") or not l.startswith("."))]
    label_at = {l[:-1]: i for i, l in enumerate(lines) if l.endswith(":")}
    loops = []
    for i, l in enumerate(lines):
        t = l.split()
        if t[0].startswith("s_cbranch") or t[0] == "s_branch":
            tgt = t[1]
            if tgt in label_at and label_at[tgt] < i:
                loops.append((label_at[tgt], i))
    for a, b in [ab for ab in loops if not any(c <= ab[0] and d >= ab[1] and (c, d) != ab for c, d in loops)]:      # the outermost loops: the row loops (everything inside them is unrolled)
        ins = [l for l in lines[a:b + 1] if not l.endswith(":")]
        ops = collections.Counter(l.split()[0] for l in ins)
        pick = lambda f: sum(v for k, v in ops.items() if f(k))
        if not any(k.startswith("global_load") for k in ops):
            continue
        print(f"{name[:48]} loop {lines[a][:-1]}: total {len(ins)}, v_mov_b64 {pick(lambda k: k.startswith('v_mov_b64'))}, v_mov_b32 {pick(lambda k: k.startswith('v_mov_b32'))} "
              f"(dpp {pick(lambda k: k.endswith('_dpp'))}), v_cndmask {pick(lambda k: k.startswith('v_cndmask'))}, ds_bpermute {ops['ds_bpermute_b32']}, "
              f"s_waitcnt {ops['s_waitcnt']}, f64 {pick(lambda k: 'f64' in k)}, v_rcp_f64 {pick(lambda k: k.startswith('v_rcp_f64'))}, global_load {pick(lambda k: k.startswith('global_load'))}, "
              f"global_store {pick(lambda k: k.startswith('global_store'))}")
        if listing:
            n = 0
            for l in ins:
                n += 1
                if l.startswith("global_") or (l.startswith("s_waitcnt") and "vmcnt" in l):
                    print(f"    {n:5d}  {l.split(';')[0].strip()}")
