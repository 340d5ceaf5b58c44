"""Timing of the walk-count intersection stage (ppa / citation2 route) on the bench workload.
Experiments only.

    python tools/walkbench.py citation2
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import argparse
    import torch
    import bench
    from ocn_amd import ops
    from ocn_amd.utils import CNState
    args = argparse.Namespace(dataset=sys.argv[1], scale=1.0, hiddim=None, predictor=None, batch=None, batches=1, innerprod=0.0)
    dev = torch.device("cuda:0")
    wl = bench.build_workload(args, dev, 0, 1)
    adj, e = wl["adj"], wl["edges"][0]
    ops.validate_indices = False
    out = []
    for two in (False, True):
        ops.walk_two_sided = two
        ws = {}
        for _ in range(3):
            st = CNState(adj, None, None, e, walk=True, ws=ws)
        torch.cuda.synchronize()
        t = []
        for _ in range(10):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); st = CNState(adj, None, None, e, walk=True, ws=ws); b.record()
            torch.cuda.synchronize()
            t.append(a.elapsed_time(b))
        t.sort()
        chk = int(st.cnt1.sum()) * 1000003 + int(st.cnt2.sum()) + int(st.wc[: int(st.off[-1])].sum()) * 7
        out.append(f"{'two-sided' if two else 'forward  '} {t[len(t) // 2] * 1e3:8.1f}us chk={chk}")
    print(" | ".join(out), "checksum", flush=True)


if __name__ == "__main__":
    main()
