"""Explaining a link at the collab shape (gin, H = 256, B = 65 536, cn5 with a trained checkpoint's ``innerprod`` = 0.37, the
graph of bench.py): one GPU process per arm, each under its own time limit, the arms alternated round by round in one call.

    (a) kernel  — ``ocn_cn_attribution`` alone on the batch's flag chain
    (b) torch   — the same quantity in torch on the GPU: the member entries listed (nonzero), their (wa, wb) formed, the rows of
                  ``h`` gathered per member entry (an nnz x H temporary) and a batched dot; the dot alone is timed as well.
                  This arm also runs the kernel once and compares both outputs with fp64 dots, entry by entry, within
                  (H + 2) u |w| sum|h g| + 1e-37 (u = 2^-24): the bound of tests/test_explain_gpu.py
    (c) explain — the whole of ``explain_links(m=8)``, next to one ``predictor(...)`` call on the same batch

    python tools/explainbench.py [--rounds 3] [--repeats 5] [--out profiles/explainbench.json]

Every child warms its call up, then times ``--repeats`` calls between two device events.  The parent prints and writes per
arm the median and the range over all calls of all rounds.  A child that ends abnormally ends the run: nothing more is started
on the GPU."""
import argparse
import json
import os
import statistics
import subprocess
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARMS = ("kernel", "torch", "explain")
TAG = "EXPLAINBENCH "
U = 2.0 ** -24


def timed(fn, repeats):
    """Milliseconds of each of ``repeats`` calls of ``fn``, between two device events on the current stream."""
    import torch
    out = []
    for _ in range(repeats):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        out.append(round(t0.elapsed_time(t1), 4))
    return out


def torch_members(st, adj, w):
    """The member entries of a batch state in torch: (flat positions, candidate, column, wa, wb)."""
    import torch
    from ocn_amd.explain import _entry_weights
    total = st.off[-1]
    q = torch.nonzero(st.flags[:total]).flatten()
    e = torch.searchsorted(st.off, q, right=True) - 1
    k = adj._col[adj._rowptr[st.src[e]] + (q - st.off[e])].long()
    c = st.wc[q].float() if st.wc is not None else torch.ones((), device=q.device)
    wa, wb = _entry_weights(st.flags[q], w[k], c)
    return q, e, k, wa, wb


def torch_dots(h, g1, g2, e, k, wa, wb):
    import torch
    hk = h[k]                                                        # the nnz x H temporary
    a1 = torch.where(wa != 0, wa * (hk * g1[e]).sum(1), torch.zeros((), device=h.device))
    a2 = torch.where(wb != 0, wb * (hk * g2[e]).sum(1), torch.zeros((), device=h.device))
    return a1, a2


def worst_ratio(h, g, e, k, wgt, got, H, chunk=1 << 16):
    """max over the entries with a non-zero weight of |got - w d_exact| / ((H + 2) u |w| sum|h g| + 1e-37), dots in fp64."""
    import torch
    worst = 0.0
    for lo in range(0, e.numel(), chunk):
        s = slice(lo, lo + chunk)
        pr = h[k[s]].double() * g[e[s]].double()
        wd = wgt[s].double()
        ratio = (got[s].double() - wd * pr.sum(1)).abs() / ((H + 2) * U * wd.abs() * pr.abs().sum(1) + 1e-37)
        live = wd != 0
        if bool(live.any()):
            worst = max(worst, float(ratio[live].max()))
    return worst


def child(a):
    sys.path.insert(0, ROOT)
    import torch
    import bench
    from ocn_amd import ops
    from ocn_amd.explain import explain_links
    from ocn_amd.utils import adjoverlap, fuse
    dev = torch.device("cuda:0")
    wl = bench.build_workload(SimpleNamespace(dataset=a.config, hiddim=None, predictor="cn5", batch=a.batch, scale=a.scale,
                                              full=False, batches=1, innerprod=a.innerprod), dev, 0, 1)
    pred, h, adj, adj2, args = wl["pred"], wl["h"], wl["adj"], wl["adj2"], wl["args"]
    e = wl["edges"][0].contiguous()
    B, H = e.shape[1], h.shape[1]
    out = {"arm": a.arm, "batch": B, "H": H, "n": wl["n"], "nnz": wl["nnz"], "max_deg": wl["max_deg"], "innerprod": a.innerprod}
    handles = lambda: (adjoverlap(adj, adj, e), adjoverlap(adj, adj2, e))
    with torch.no_grad():
        if a.arm == "explain":
            edges = e.t().contiguous()
            run = lambda: explain_links(pred, h, adj, adj2, edges, m=8, args=args)
            score = lambda: pred(h, adj, *handles(), e)
            for _ in range(2):
                run(); score()
            torch.cuda.synchronize()
            out["ms"] = timed(run, a.repeats)
            out["ms_predictor_call"] = timed(score, a.repeats)
        else:
            st = fuse(*handles(), e, None, adj=adj)
            w = pred._weights(st, args)
            gen = torch.Generator().manual_seed(1)
            g1, g2 = torch.randn(B, H, generator=gen).to(dev), torch.randn(B, H, generator=gen).to(dev)
            kernel = lambda: ops.cn_attribution(adj._rowptr, adj._col, st.src, st.off, st.flags, st.wc, w, h, g1, g2, order=st.order)
            attr, _ = kernel()
            st.check_status()
            q, em, k, wa, wb = torch_members(st, adj, w)
            out.update(positions=int(st.off[-1]), members=int(q.numel()), fetched=int(((wa != 0) | (wb != 0)).sum()))
            if a.arm == "kernel":
                ws = {}
                kernel = lambda: ops.cn_attribution(adj._rowptr, adj._col, st.src, st.off, st.flags, st.wc, w, h, g1, g2,
                                                    order=st.order, wsd=ws)       # (its outputs allocated once, as a predictor's scratch is)
                for _ in range(3):
                    kernel()
                torch.cuda.synchronize()
                out["ms"] = timed(kernel, a.repeats)
            else:
                whole = lambda: torch_dots(h, g1, g2, *torch_members(st, adj, w)[1:])
                dots = lambda: torch_dots(h, g1, g2, em, k, wa, wb)
                for _ in range(3):
                    whole(); dots()
                torch.cuda.synchronize()
                out["ms"] = timed(whole, a.repeats)
                out["ms_dot_only"] = timed(dots, a.repeats)
                a1, a2 = dots()
                ratios = {"kernel": max(worst_ratio(h, g1, em, k, wa, attr[q, 0], H), worst_ratio(h, g2, em, k, wb, attr[q, 1], H)),
                          "torch": max(worst_ratio(h, g1, em, k, wa, a1, H), worst_ratio(h, g2, em, k, wb, a2, H))}
                out["worst_error_over_bound"] = ratios
                out["outputs_agree_within_bound"] = bool(ratios["kernel"] <= 1.0 and ratios["torch"] <= 1.0)
    print(TAG + json.dumps(out), flush=True)


def spread(t):
    return dict(median=statistics.median(t), min=min(t), max=max(t), calls=t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arm", choices=ARMS, help="(internal) run one arm in this process")
    ap.add_argument("--config", default="collab")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--batch", type=int, default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--innerprod", type=float, default=0.37)
    ap.add_argument("--arms", default=",".join(ARMS))
    ap.add_argument("--limit", type=int, default=240, help="seconds one child may take")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.arm:
        return child(a)
    keys = ("ms", "ms_dot_only", "ms_predictor_call")
    runs = {arm: {} for arm in a.arms.split(",")}
    meta = {}
    for rnd in range(a.rounds):
        for arm in runs:
            cmd = [sys.executable, os.path.abspath(__file__), "--arm", arm, "--config", a.config, "--scale", str(a.scale),
                   "--repeats", str(a.repeats), "--innerprod", str(a.innerprod)] + (["--batch", str(a.batch)] if a.batch else [])
            try:
                p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
            except subprocess.TimeoutExpired:
                print(f"arm {arm} round {rnd}: over its {a.limit} s limit; stopping", flush=True)
                return 2
            line = [l for l in p.stdout.splitlines() if l.startswith(TAG)]
            if p.returncode != 0 or not line:
                print(f"arm {arm} round {rnd}: exit status {p.returncode}; stopping\n{p.stderr[-2000:]}", flush=True)
                return 2
            r = json.loads(line[-1][len(TAG):])
            for key in keys:
                if key in r:
                    runs[arm].setdefault(key, []).extend(r.pop(key))
            meta[arm] = r
            print(f"round {rnd} {arm:8s}: " + ", ".join(f"{key} median {statistics.median(t[-a.repeats:]):.4f}"
                                                          for key, t in runs[arm].items()), flush=True)
    out = {"workload": f"{a.config}-shaped synthetic graph of bench.py, cn5 with innerprod = {a.innerprod}, ONE batch; ms per call "
                       "between device events after a warm-up; kernel: ocn_cn_attribution alone; torch: the same quantity with "
                       "gathered rows of h and a batched dot (ms: from the flags; ms_dot_only: gather + dot with the member list "
                       "given); explain: explain_links(m=8) beside one predictor call (ms_predictor_call)",
           "rounds": a.rounds, "repeats": a.repeats,
           "arms": {arm: dict(**{key: spread(t) for key, t in r.items()}, **meta[arm]) for arm, r in runs.items()}}
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
