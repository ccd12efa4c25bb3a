"""Split a rocprofv3 kernel-trace (.db) of the SL step into 3x3 forward / dgrad / 5x5 conv and
wgrad launch averages (forward = conv launches before the step's first wgrad launch; direct
conv_tap_pp and Winograd conv_wino launches alike), the idle gap between consecutive forward
conv_wino launches, and the chained forward (conv_wino_chain_kernel: one launch for a run of
layers) as time per launch and per layer.

    python tools/convsplit.py [--chain-layers 11] <trace dir>/sl_results.db [...]

--chain-layers: layers per chain launch (the kernel's name does not carry it; the north-star
trunk chains its 11 3x3 layers).
"""
import re
import sqlite3
import statistics as st
import sys


def split(path, chain_layers=11):
    db = sqlite3.connect(path)
    cols = [r[1] for r in db.execute("pragma table_info(kernels)")]
    nc = 'kernel_name' if 'kernel_name' in cols else 'name'
    fw, dg, f5, wg, ch, gaps = [], [], [], [], [], []
    state = 'f'
    last_fw_end = None  # end of the previous launch if it was a forward conv_wino launch
    for n, s, e in db.execute("select %s, start, end from kernels order by start" % nc):
        d = (e - s) / 1e3
        prev_end, last_fw_end = last_fw_end, None
        if 'conv_wino_chain_kernel' in n:
            ch.append(d)
            continue
        if 'wgrad_slab_kernel' in n:
            state = 'b'
            wg.append(d)
            continue
        if 'conv_wino_kernel' in n:
            (fw if state == 'f' else dg).append(d)
            if state == 'f':
                if prev_end is not None:
                    gaps.append((s - prev_end) / 1e3)
                last_fw_end = e
            continue
        m = re.search(r'conv_tap_pp_kernel<([^>]*)>', n)
        if not m:
            continue
        a = [x.strip() for x in m.group(1).split(',')]
        if a[3] == '5':  # <NB, NT, BNP, KS, ...> (round 5 template)
            f5.append(d)
            state = 'f'
            continue
        (fw if state == 'f' else dg).append(d)
    mean = lambda v: st.mean(v) if v else float('nan')
    med = lambda v: st.median(v) if v else float('nan')
    out = ("fwd3x3 %.2f us (median %.2f, n=%d)  dgrad %.2f us (median %.2f, n=%d)  5x5 %.2f us"
           "  wgrad %.2f us (n=%d)" % (mean(fw), med(fw), len(fw), mean(dg), med(dg), len(dg),
                                      mean(f5), mean(wg), len(wg)))
    if gaps:
        out += "  fwd wino gap %.2f us (median %.2f, n=%d)" % (mean(gaps), med(gaps), len(gaps))
    if ch:
        out += ("  fwd chain %.2f us (median %.2f, n=%d) = %.2f us per layer of %d"
                % (mean(ch), med(ch), len(ch), med(ch) / chain_layers, chain_layers))
    return out


if __name__ == "__main__":
    args = sys.argv[1:]
    layers = 11
    if args and args[0] == "--chain-layers":
        layers = int(args[1])
        args = args[2:]
    for p in args:
        print(p, split(p, layers))
