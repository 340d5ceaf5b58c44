#!/usr/bin/env python
"""Headline benchmark: candidate edges / second through the CN predictor forward on a synthetic graph
of an OGB dataset's shape.  Default = BASELINE.json configs[1]: ogbl-collab shape, gin, hiddim 256,
cn5, batch 65536 (README.md:42 of the reference).

A step = one candidate batch through the hot path exactly as ``test()`` runs it
(NeighborOverlap_large.py:121-159): the CN builder (adjoverlap(A, A, e) + adjoverlap(A, A², e), or
get_cn1_cn2(A, e) on the pygho route), then the predictor forward (intersection -> column weights ->
pooling -> MLP heads), with the encoder output h and A² computed once per graph outside the timed
region and everything resident in HBM.  The predictor is built the way the reference drivers build it
(NeighborOverlap_large.py:272-276,297-298: for cn5 / cn7 only ``cndeg`` is forwarded, so --use_xlin /
--tailact / --beta of the README commands are dead flags and the head is 9 Linear(H,H) + Linear(H,1)).
The timed steps rotate over ``--batches`` (8) distinct seeded candidate batches, whose ids were
bounds-checked once before the timed region (what ``pipeline.score_edges`` does for a whole split);
``value_validate_per_batch`` is the same loop with the per-batch check (one host sync per batch) left on.

A plain run sets up, warms up, times the K steps and prints the headline line (``metric``, ``value``, ``unit``,
``ms_per_step``, ...).  Everything else it can measure or check — stage timers and roofline objects, repeats of the
timed loop, the one-stream / per-batch-validation / trained-innerprod legs, the CPU baseline and its parity check, the
encoder timing — runs only with ``--full``.  ``--dump-outputs DIR`` writes the scores of the last timed step as
``DIR/scores.npy`` (float32; the inputs are seeded, so two builds can be compared output for output).

    python bench.py --gpus 1 --steps 128 --warmup 8
    python bench.py --full                      # the headline line plus every other figure and check
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W
    python bench.py --config citation2          # other BASELINE configs: citation2 | ppa | ddi | cora

N > 1: one process per GPU; graph / h / weights replicated, each rank owns a ``batch``-edge slice of
a global batch of N x batch (weak scaling); per step one RCCL all-reduce of the packed column
histograms and one all-gather of the scores (ocn_amd/dist.py).
"""
import argparse
import glob
import json
import os
import sys
import time
from functools import partial
from types import SimpleNamespace

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12       # B/s, MI355X spec (MI355X_MICROARCH.md: 8.0 TB/s spec, 6.29 TB/s measured copy)
F32_MFMA_PEAK = 157.3e12    # FLOP/s, dense f32-in/f32-acc MFMA (same guide, chip-level table)
BF16_MFMA_PEAK = 2.5e15     # FLOP/s, dense bf16 MFMA

# the reference's README commands (README.md:27,42,47,92,98): encoder class, conv, layers, hiddim, predictor
# (BASELINE.json's), CN route, batch, ids-as-features, args.sum, and the flags each command sets: --ln (encoder
# LayerNorm), --lnnn (predictor LayerNorm), --res, --jk, --nnlayers, --predp, --preedp
CONFIGS = {
    "collab":    dict(enc="GCN",  conv="gin",     layers=1, H=256, pred="cn5", route="adj2",  batch=65536, ids=False, sum=1.0,
                      ln=True,  lnnn=True,  res=False, jk=True,  nnlayers=3, predp=0.05, preedp=0.4),
    "cora":      dict(enc="GCN",  conv="puregcn", layers=1, H=256, pred="cn5", route="adj2",  batch=1152,  ids=False, sum=0.0,
                      ln=True,  lnnn=True,  res=False, jk=True,  nnlayers=3, predp=0.05, preedp=0.4),
    "ppa":       dict(enc="GCN2", conv="gcn",     layers=1, H=64,  pred="cn5", route="walk",  batch=2048,  ids=True,  sum=0.0,
                      ln=True,  lnnn=True,  res=False, jk=True,  nnlayers=3, predp=0.0,  preedp=0.0),
    "citation2": dict(enc="GCN3", conv="gcn",     layers=5, H=32,  pred="cn7", route="walk",  batch=2048,  ids=False, sum=1.0,
                      ln=True,  lnnn=False, res=True,  jk=True,  nnlayers=3, predp=0.10, preedp=0.12),
    "ddi":       dict(enc="GCN",  conv="puregcn", layers=3, H=64,  pred="cn7", route="block", batch=32768, ids=True,  sum=2.74,
                      ln=False, lnnn=True,  res=True,  jk=False, nnlayers=3, predp=0.10, preedp=0.13),
}


def head_layout(pred) -> str:
    """'xcn1lin 3 + xcn2lin 3 + xijlin 2 + lin 1 Linear(H,H) + Linear(H,1)' read off the module."""
    import torch.nn as nn
    parts, tot = [], 0
    for name in ("xcn1lin", "xcn2lin", "xijlin", "lin"):
        seq = getattr(pred, name)
        hh = sum(1 for m in seq if isinstance(m, nn.Linear) and m.out_features == m.in_features)
        tail = sum(1 for m in seq if isinstance(m, nn.Linear) and m.out_features == 1)
        lns = sum(1 for m in seq if isinstance(m, nn.LayerNorm))
        tot += hh
        parts.append(f"{name}: {hh} Linear(H,H)" + (f" + Linear(H,1)" if tail else "") + (f", {lns} LayerNorm" if lns else ""))
    return f"{tot} Linear(H,H) + dot per edge [" + "; ".join(parts) + "]"


class StageTimer:
    """HIP events on the stream each ocn_* kernel is launched on.  ``mark(name)`` records an event on torch's CURRENT stream
    and remembers which stream that was; a stage's duration is the distance between two consecutive marks OF THE SAME
    STREAM — the scoring loop runs phase A (prep, intersection, weights, class order) on side streams and phase B (pooling,
    heads) on the caller's, and an interval that starts at one stream's event and ends at another's measures nothing
    (VERDICT r3 #4).  Every phase opens with a "begin" mark on its own stream, so a stage interval never spans two phases."""

    # the stages the line's roofline objects need; the small phase-A kernels (weights, class order, schedule) are timed with
    # --all-stages only: every recorded event costs the timed region (16 marks per sampled step: -5 % on the driver's
    # 20-step run, measured; these 9: -2 %)
    LEAN = frozenset(("begin", "cn_prep", "cn_flags", "cn_pre", "cn_gather", "mlp_glue", "linear", "allreduce_hist"))

    def __init__(self, pool=0, lean=True):
        self.events = []
        self.lean = lean
        self.active = True
        self.flops = {}
        self.sampled_steps = 0
        # hipEventCreate is the expensive part on a busy host: create the events before the timed
        # region, only record() inside it
        self.pool = [torch.cuda.Event(enable_timing=True) for _ in range(pool)]
        for ev in self.pool:                   # torch creates the hipEvent lazily, at the first record()
            ev.record()
        self._raw = getattr(torch._C, "_cuda_getCurrentRawStream", None)

    def mark(self, name, flops=0.0):
        if not self.active or (self.lean and name not in self.LEAN):
            return
        self.flops[name] = self.flops.get(name, 0.0) + flops
        ev = self.pool.pop() if self.pool else torch.cuda.Event(enable_timing=True)
        sid = self._raw(torch._C._cuda_getDevice()) if self._raw else torch.cuda.current_stream().cuda_stream
        ev.record()
        self.events.append((name, ev, sid))

    def totals(self):
        """{stage: (mean ms per launch, launches, ms per sampled step)} from same-stream pairs only."""
        tot, prev = {}, {}
        for name, ev, sid in self.events:
            p = prev.get(sid)
            if name != "begin" and p is not None:
                tot.setdefault(name, []).append(p.elapsed_time(ev))
            prev[sid] = ev
        n = max(self.sampled_steps, 1)
        return {k: (sum(v) / len(v), len(v), sum(v) / n) for k, v in tot.items()}


def sampled_step(it, steps):
    """Stage events are recorded on 8 steps of the timed region whatever --steps is (all but the first when there are fewer),
    evenly spread, never on step 0: with three batches in flight step 0 PRIMES the pipeline (three phase-A passes are
    enqueued before its phase B), every later step enqueues exactly one phase A (of batch it + 2) and one phase B (of batch it)."""
    if steps <= 9:
        return it > 0
    return it in {1 + (q * (steps - 2)) // 7 for q in range(8)}


def make_predictor(cfg, dev):
    """predfn = partial(predictor_dict[name], cndeg=args.cndeg); predfn(hiddim, hiddim, 1, nnlayers, predp,
    preedp, lnnn) — NeighborOverlap_large.py:272-276,297-298 (same in the ppa / citation2 drivers)."""
    import ocn_amd.model as M
    H = cfg["H"]
    predfn = partial(M.predictor_dict[cfg["pred"]], cndeg=-1)
    return predfn(H, H, 1, cfg["nnlayers"], cfg["predp"], cfg["preedp"], cfg["lnnn"]).to(dev).eval()


def build_workload(args, dev, rank, world):
    import ocn_amd.model as M
    from ocn_amd.sparse import SparseTensor
    from ocn_amd.synth import dataset_like, sample_edges
    from ocn_amd.utils import sparse_tensor_multiply

    cfg = dict(CONFIGS[args.dataset])
    cfg["H"] = args.hiddim or cfg["H"]
    cfg["pred"] = args.predictor or cfg["pred"]
    cfg["batch"] = args.batch or cfg["batch"]
    H = cfg["H"]
    t0 = time.time()
    ei, n, shape = dataset_like(args.dataset, seed=0, scale=args.scale)
    adj = SparseTensor.from_edge_index(ei.to(dev), sparse_sizes=(n, n), trust_data=True).to_symmetric()
    del ei
    torch.cuda.synchronize()
    t_graph = time.time() - t0
    torch.manual_seed(0)
    if cfg["ids"]:
        x, fin, max_x = torch.arange(n, device=dev), H, n
    else:
        fin, max_x = (shape["feat"] or H), -1
        x = torch.randn(n, fin, device=dev)
    enc = getattr(M, cfg["enc"])(fin, H, H, cfg["layers"], 0.05, cfg["ln"], cfg["res"], max_x, cfg["conv"], cfg["jk"], 0.0,
                                 xdropout=0.7, taildropout=0.3).to(dev).eval()
    pred = make_predictor(cfg, dev)
    if getattr(args, "innerprod", 0.0):
        pred.innerprod.fill_(args.innerprod)           # a trained checkpoint's buffer (order-exact S2 path of cn5)
    t_enc = None
    with torch.no_grad():
        h = enc(x, adj)
        if getattr(args, "full", True):                   # (the encoder's time is a --full figure)
            torch.cuda.synchronize()
            t0 = time.time()
            for _ in range(3):
                h = enc(x, adj)
            torch.cuda.synchronize()
            t_enc = (time.time() - t0) / 3
    adj2, t_a2 = None, 0.0
    if cfg["route"] != "walk":
        t0 = time.time()
        if cfg["route"] == "block":
            adj2 = sparse_tensor_multiply(adj, 1024)
        else:
            with torch.no_grad():                         # (the drivers' test() is @torch.no_grad(): the whole product, not the training step's rows on demand)
                sp = adj.to_torch_sparse_coo_tensor()
                adj2 = SparseTensor.from_torch_sparse_coo_tensor(sp @ sp, False)
        torch.cuda.synchronize()
        t_a2 = time.time() - t0
    r, c, _ = adj.coo()
    rc, cc = r.cpu(), c.cpu()
    # `batches` global batches of world x B edges each, seeded 1, 2, ...; rank r owns slice r of each
    per_rank = 1 if getattr(args, "scaling", "weak") == "strong" else world          # strong scaling: the configuration's one batch, cut over the ranks
    edges = [sample_edges(rc, cc, n, cfg["batch"] * per_rank, seed=1 + b).to(dev) for b in range(max(getattr(args, "batches", 1), 1))]
    return dict(cfg=cfg, n=n, adj=adj, adj2=adj2, h=h.contiguous(), pred=pred, edges=edges, enc_s=t_enc, a2_s=t_a2,
                graph_s=t_graph, nnz=adj.nnz(), nnz2=adj2.nnz() if adj2 is not None else None,
                max_deg=adj.max_rowcount(), args=SimpleNamespace(sum=cfg["sum"]))


def cn_handles(wl, e):
    from ocn_amd.utils import adjoverlap, get_cn1_cn2
    if wl["cfg"]["route"] == "walk":
        return get_cn1_cn2(wl["adj"], e)
    return adjoverlap(wl["adj"], wl["adj"], e), adjoverlap(wl["adj"], wl["adj2"], e)


def batch_bytes(wl, mine, H):
    """Byte counts of one candidate batch, per kernel.

    ``formula``: SURVEY.md §8(d), bytes(e) = 4(d_i+d_j) + 4 d2_j + 4H(c1+c2) + 8H + 28 — one embedding row per CN
    entry, the whole A² row of j.  ``compulsory``: what a kernel with an ideal cache has to move for this batch —
    every DISTINCT embedding row / weight row once, the CSR rows it walks once, its outputs once; on the walk
    route the rows of the cheaper endpoint's neighbours (what the two-sided sweep enumerates), not Σ_{k∈N(i)} d_k.
    ``achieved`` in the roofline objects is compulsory bytes / time (never above the HBM peak by construction of
    an ideal-cache count); the formula figure is printed beside it."""
    from ocn_amd.utils import CNState
    adj = wl["adj"]
    rp = adj._rowptr
    deg = rp[1:] - rp[:-1]
    src, dst = mine[0], mine[1]
    B = mine.shape[1]
    walk = wl["cfg"]["route"] == "walk"
    st = CNState(adj, None, None, mine, walk=True) if walk else CNState(adj, adj, wl["adj2"], mine)
    cnt1, cnt2 = st.cnt1, st.cnt2
    di, dj = deg[src], deg[dst]
    sdi, sdj = int(di.sum()), int(dj.sum())
    c12 = int(cnt1.sum()) + int(cnt2.sum())
    hc = st.hist_counts()
    touched_cols = int((hc[:, 2] > 0).sum())                       # distinct columns with a union entry
    rows_h = torch.zeros(wl["n"], dtype=torch.bool, device=mine.device)
    rows_h[hc[:, 2] > 0] = True
    rows_h[src] = True
    rows_h[dst] = True
    distinct_h = int(rows_h.sum())
    has_any = (cnt1 > 0) | (cnt2 > 0)
    pooled_rows_walked = int(di[has_any].sum())                    # rows without an entry are not walked
    if walk:
        nds = adj.neighbor_degree_sum()
        ndi, ndj = nds[src], nds[dst]
        rev = (dj > 0) & (di > 0) & ((2 * ndj + di * ((dj + 15) // 16) + 2 * di) < ndi)     # csrc/common.h walk_reverse
        swept = int(torch.where(rev, ndj, ndi).sum())
        second_formula = int(ndi.sum())
        flags_formula = 4 * (sdi + sdj) + 4 * second_formula + 24 * B
        flags_comp = 4 * (sdi + sdj) + 4 * swept + 5 * sdi + 24 * B          # + flag byte and walk count per position
    else:
        rp2 = wl["adj2"]._rowptr
        second_formula = int((rp2[dst + 1] - rp2[dst]).sum())
        flags_formula = 4 * (sdi + sdj) + 4 * second_formula + 24 * B
        bm = wl["adj2"]._bitmap
        probe = (4 * sdi if bm is not None else 0)                 # one 4-byte word of the bit row per neighbour of i
        flags_comp = 4 * (sdi + sdj) + (probe if bm is not None else 4 * second_formula) + sdi + 16 * touched_cols + 24 * B
    gather_formula = 4 * H * c12 + 8 * H * B + 4 * B
    n_w1 = int((cnt1 > 0).sum())
    gather_comp = (4 * H * distinct_h + 16 * touched_cols + 5 * pooled_rows_walked
                   + 4 * H * (n_w1 + int(has_any.sum()) + B) + 24 * B)
    return dict(flags_formula=flags_formula, flags_compulsory=flags_comp, gather_formula=gather_formula,
                gather_compulsory=gather_comp, mean_di=sdi / B, mean_dj=sdj / B, mean_second=second_formula / B,
                mean_c1=cnt1.float().mean().item(), mean_c2=cnt2.float().mean().item(),
                distinct_h_rows=distinct_h, touched_cols=touched_cols,
                frac_rows_cn1=n_w1 / B, frac_rows_any=float(has_any.float().mean()),
                n_cn1=n_w1, n_any=int(has_any.sum()), n_cn2=int((cnt2 > 0).sum()))


def cpu_baseline(wl, args, mine):
    """The oracle (a port of the reference's op sequence on torch CPU ops, oracle/ocn_oracle.py) timed on the
    host cores of this box on the step's FULL candidate batch (or --cpu-sample edges of it), the adjacency's
    rowptr cached as torch_sparse caches it.  The thread count is swept on a 1/8 sample (8 / 32 / 64 / all the
    cores this process may use) and the full batch is then timed once with the fastest."""
    from oracle import ocn_oracle as O
    ncores = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else os.cpu_count()
    cfg, adj, adj2 = wl["cfg"], wl["adj"], wl["adj2"]
    r, c, _ = adj.coo()
    oadj = O.SpM(r.cpu(), c.cpu(), None, wl["n"], wl["n"])
    oadj.rowptr()
    oadj2 = None
    if adj2 is not None:
        r2, c2, _ = adj2.coo()
        oadj2 = O.SpM(r2.cpu(), c2.cpu(), None, wl["n"], wl["n"])
        oadj2.rowptr()
    h = wl["h"].cpu()
    sd = {k: v.detach().cpu() for k, v in wl["pred"].state_dict().items()}

    def run(b):
        e = mine[:, :b].cpu()
        t0 = time.time()
        if oadj2 is None:
            cn1, cn2 = O.get_cn1_cn2(oadj, e)
        else:
            cn1, cn2 = O.adjoverlap(oadj, oadj, e), O.adjoverlap(oadj, oadj2, e)
        if cfg["pred"] == "cn5":
            out = O.cn5_forward(sd, h, cn1, cn2, e, ln=cfg["lnnn"])
        else:
            out = O.cn7_forward(sd, h, cn1, cn2, e, cfg["sum"], ln=cfg["lnnn"])
        return time.time() - t0, out

    full = mine.shape[1] if not args.cpu_sample else min(args.cpu_sample, mine.shape[1])
    probe = max(full // 8, min(full, 256))
    sweep = {}
    for nt in sorted({t for t in (8, 32, 64, ncores) if t <= ncores} | {min(8, ncores)}):
        torch.set_num_threads(nt)
        run(min(probe, 256))                              # thread pool warm-up
        sweep[nt] = probe / run(probe)[0]
    best = max(sweep, key=sweep.get)
    torch.set_num_threads(best)
    t, out = run(full)
    builder = "get_cn1_cn2" if oadj2 is None else "adjoverlap x2"
    model = "unknown"
    try:
        with open("/proc/cpuinfo") as f:
            model = next((l.split(":", 1)[1].strip() for l in f if l.startswith("model name")), "unknown")
    except OSError:
        pass
    return dict(value=full / t, unit="edges/s", cores=best, kind="port", cpu_model=model, usable_cores=ncores,
                sample=f"the step's {'full ' if full == mine.shape[1] else ''}{full}-edge batch as one batch, "
                       f"oracle/ocn_oracle.py {builder} + {cfg['pred']}_forward (rowptr cached), {t:.2f} s with {best} torch "
                       f"threads of {ncores} usable cores; thread sweep on {probe} edges: "
                       + ", ".join(f"{k}t {v:.0f} e/s" for k, v in sorted(sweep.items()))), full, out


def pmc_traffic(dataset, kernel_substr):
    """HBM-side bytes per launch of a kernel from the committed PMC passes (profiles/r*_pmc_<config>.json, or
    r*_pmc.json for the default config: separate rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE runs of this command).
    FETCH_SIZE is doubled (gfx950 counts 128-B requests as 64 B — MI355X_MICROARCH.md §HBM; calibrated on
    rows_ln_relu / combine3 whose byte counts are known exactly), both are in KiB."""
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", f"r*_pmc_{dataset}.json")))
    if not files and dataset == "collab":
        files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc.json")))
    if not files:
        return None
    best = None
    for k, v in json.load(open(files[-1])).items():
        if kernel_substr in k and "FETCH_SIZE" in v and "WRITE_SIZE" in v:
            t = (2.0 * v["FETCH_SIZE"]["avg"] + v["WRITE_SIZE"]["avg"]) * 1024.0
            best = t if best is None else max(best, t)
    return best


DUMP_MAX_BYTES = 64 << 20


def dump_outputs(path, scores):
    """--dump-outputs: the scores the last timed step returned, as <path>/scores.npy in float32 — or, above 64 MB, the rows of a
    fixed seeded sample of them in ascending order, with their row ids as <path>/scores_rows.npy (float64)."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    s = scores.detach().float().cpu()
    if s.numel() * 4 > DUMP_MAX_BYTES:
        keep = DUMP_MAX_BYTES // (8 + 4 * s[0].numel())            # a float64 row id + the row's float32 scores
        rows = torch.randperm(s.shape[0], generator=torch.Generator().manual_seed(0))[:keep].sort().values
        s = s[rows]
        np.save(os.path.join(path, "scores_rows.npy"), rows.double().numpy())
    np.save(os.path.join(path, "scores.npy"), s.numpy())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--config", "--dataset", dest="dataset", default="collab", choices=sorted(CONFIGS))
    ap.add_argument("--predictor", default=None)
    ap.add_argument("--batch", type=int, default=None)
    ap.add_argument("--hiddim", type=int, default=None)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--batches", type=int, default=8, help="distinct seeded candidate batches the timed steps rotate over")
    ap.add_argument("--innerprod", type=float, default=0.0, help="value of the predictor's innerprod buffer (0 = fresh model)")
    ap.add_argument("--cpu-sample", type=int, default=0, help="edges of the batch the CPU baseline runs (0 = the full batch)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-stage-timers", action="store_true")
    ap.add_argument("--no-validate-leg", action="store_true", help="skip the second timed loop with the per-batch id check on")
    ap.add_argument("--scaling", choices=("weak", "strong"), default="weak",
                    help="N > 1: weak = `batch` candidates PER RANK of a global batch of N x batch (the default line); strong = the "
                         "reference's ONE batch (collab: 65 536 edges) cut N ways, north_star's 'partition the edge batch across the GPUs'")
    ap.add_argument("--no-graph-loops", action="store_true", help="N = 1: enqueue every step launch by launch (no HIP-graph replay of the phases)")
    ap.add_argument("--no-one-stream-leg", action="store_true",
                    help="skip the untimed pass with the streams serialised (the *_one_stream keys): a kernel trace of the command "
                         "then averages over the overlapped loop only, like the line's own stage events")
    ap.add_argument("--graph", action="store_true",
                    help="replay the step as a captured HIP graph (pipeline.GraphedScorer; one GPU, no stage events: "
                         "the roofline objects are then null)")
    ap.add_argument("--prewarm", type=int, default=64, help="untimed runtime pre-warm steps before --warmup")
    ap.add_argument("--run-ahead", type=int, default=6, help="steps the host may enqueue ahead of the GPU")
    ap.add_argument("--timer-every", type=int, default=0, help="record stage events on every n-th timed step (0 = steps // 8: at least 8 sampled steps)")
    ap.add_argument("--all-stages", action="store_true", help="stage events for every kernel group of the step (default: the intersection, "
                    "pooling and heads launches only — each recorded event costs the timed region)")
    ap.add_argument("--repeats", type=int, default=3, help="times the timed loop runs in all; `value` is the first run, the others are reported beside it")
    ap.add_argument("--rehearse-collectives", action="store_true",
                    help="one rank, but with the N > 1 code path: RCCL process group, histogram all-reduce and score "
                         "all-gather executed (a one-GPU box can then time what the collectives add); not a bench line")
    ap.add_argument("--full", action="store_true",
                    help="beyond the headline figure: stage timers and roofline objects, --repeats, the one-stream, per-batch "
                         "validation and trained-innerprod legs, the CPU baseline with its parity check, the encoder timing "
                         "(the --no-* switches above act on these)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the scores of the last timed step as DIR/scores.npy (float32)")
    args = ap.parse_args()

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: launch with torch.distributed.run")
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    import torch.distributed as dist
    if world > 1:
        dist.init_process_group("nccl", device_id=dev)
    elif args.rehearse_collectives:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29517")
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
        import ocn_amd.dist as _d
        _d.force_collectives = True

    from ocn_amd import _lib, ops
    from ocn_amd.dist import gather_scores, shard_bounds
    _lib.lib()                                     # no HIP extension -> no benchmark

    wl = build_workload(args, dev, rank, world)
    cfg, pred, h, adj = wl["cfg"], wl["pred"], wl["h"], wl["adj"]
    H = cfg["H"]
    is_default = args.scale == 1.0 and not (args.predictor or args.batch or args.hiddim or args.innerprod)
    pmc = partial(pmc_traffic, args.dataset) if is_default else (lambda k: None)
    B_total = wl["edges"][0].shape[1]
    s, e = shard_bounds(B_total, world)[rank]
    mines = [g[:, s:e].contiguous() for g in wl["edges"]]
    NB = len(mines)
    pred.set_edge_sharding(None, enabled=world > 1 or args.rehearse_collectives)

    pending = [None]                               # the previous batch's score all-gather (N > 1), still in flight
    pattern = ["single rank: no collective"]          # the communication pattern of the timed loop, reported in the JSON line
    # N > 1: two batches in flight — the intersection pass of batch t + 1 is enqueued before batch t waits for its
    # histogram all-reduce (predictor.begin / .finish), so the collective runs beside compute instead of stalling the
    # stream.  The timed loop still begins and finishes exactly K batches between its barriers.
    pipelined = not args.graph                     # N = 1 too: phase A of batch t + 1 runs on a second stream beside phase B of batch t
    ahead = [None, -1]                             # [token of the batch already begun, its index]

    # N = 1: the library's loops replay phase A / phase B of a scratch set as captured HIP graphs (pipeline.GraphedPhases: the host
    # side of a step, ~25 ctypes launches, becomes one id copy and two graph launches); steps whose stages are being timed run
    # launch by launch.  A new set of graphs whenever the predictor's state changes what is launched (the trained-innerprod leg).
    use_graphs = (world == 1 and not args.rehearse_collectives and not args.no_graph_loops and not args.graph and ops.graph_loops)
    graphed = [None]

    def new_graphs():
        from ocn_amd.pipeline import GraphedPhases
        graphed[0] = GraphedPhases(pred, h, adj, lambda e: cn_handles(wl, e), mines[0].shape[1], wl["args"]) if use_graphs else None

    def begin(it):
        mine = mines[it % NB]
        if graphed[0] is not None:
            return graphed[0].begin(it, mine)
        c1, c2 = cn_handles(wl, mine)
        return pred.begin(h, adj, c1, c2, mine, slot=it, args=wl["args"])

    def finish(tok):
        if graphed[0] is not None:
            return graphed[0].finish(tok).clone()            # (a replay's scores live in the graph's pool until the set's next batch)
        return pred.finish(h, tok, wl["args"])

    def step(it=0, last=True):
        with torch.no_grad():
            mine = mines[it % NB]
            if pipelined:
                tok = ahead[0] if ahead[1] == it else begin(it)
                ahead[0], ahead[1] = (None, -1) if last else (begin(it + 1), it + 1)
                loc = pred.finish(h, tok, wl["args"])
            else:
                c1, c2 = cn_handles(wl, mine)
                loc = pred(h, adj, c1, c2, mine, wl["args"])
            # warm-up / validation steps: gather per batch; the all-gather of batch t runs beside batch t + 1 (its own stream)
            if pending[0] is not None:
                pending[0].wait()
            out, pending[0] = gather_scores(loc, B_total, async_op=True)
            return out

    for b in range(NB):                            # every batch validated once (bounds check + flag capacity)
        out = step(b)
    torch.cuda.synchronize()
    ops.validate_indices = False                   # ids checked above, as pipeline.score_edges does for a whole split
    if args.graph:
        if world > 1:
            raise SystemExit("--graph is a single-GPU option")
        from ocn_amd.pipeline import GraphedScorer
        scorer = GraphedScorer(pred, h, adj, wl.get("adj2"), mines[0].shape[1], wl["args"],
                               route="walk" if cfg["route"] == "walk" else "pattern")
        eager_step = step

        def step(it=0, last=True):
            return scorer(mines[it % NB])
        for b in range(NB):
            assert torch.equal(step(b), eager_step(b))
        args.no_stage_timers = True
    # Runtime pre-warm (untimed, before the W warm-up steps): the HIP runtime grows its internal
    # command/signal pools in ~35 ms host stalls during the first ~1000 launches of a process; a short
    # --warmup would otherwise put one of them inside the timed region.
    new_graphs()
    if pipelined and args.prewarm > 0:             # (on the timed loop's own code path too: what a kernel trace of this command averages
        from ocn_amd.pipeline import pipelined_shard_loop           # over is then the overlapped loop, not a one-stream variant of it)
        with torch.no_grad():
            for _ in range(max(args.prewarm // 16, 1)):
                pipelined_shard_loop(begin, finish, 16, B_total, gather_at_end=True)
                torch.cuda.synchronize()
    else:
        for i in range(args.prewarm):
            step(i)
            if i % 4 == 3:
                torch.cuda.synchronize()
    if pipelined and args.warmup > 0:              # the W warm-up steps run the timed loop's own code path (second stream included)
        from ocn_amd.pipeline import pipelined_shard_loop
        with torch.no_grad():
            pipelined_shard_loop(begin, finish, args.warmup, B_total, gather_at_end=True)
        torch.cuda.synchronize()
    else:
        for i in range(args.warmup):
            step(i)

    def timed_loop(steps, timer, overlap=None):
        """EXACTLY `steps` steps between two barrier + synchronize brackets; returns (seconds, host enqueue seconds)."""
        ops.stage_timer = timer
        # Python's cycle collector stays out of the timed region: a generation-2 pass over a process that holds a few hundred
        # thousand torch objects is a 50 - 150 ms pause (measured in the training loop) — several times a 13 ms region
        import gc
        gc.collect()
        gc.disable()
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()
        # Flow control: the host enqueues a step several times faster than the GPU runs it.  Left alone, the
        # HIP runtime lets ~1000 commands pile up and then blocks the host until the queue has drained
        # completely (measured: 35 ms stalls, GPU idle at the end of each) — so the host waits on the event of
        # the step `run_ahead` steps back, as a real scoring loop that consumes its scores would.
        run_ahead = max(args.run_ahead, 1)
        ring = [torch.cuda.Event() for _ in range(run_ahead)]
        for ev in ring:
            ev.record()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        t_wait = 0.0
        out = None
        t_waits = [0.0]

        def before_step(it):
            tw = time.perf_counter()
            ring[it % run_ahead].synchronize()
            t_waits[0] += time.perf_counter() - tw
            if timer:                                  # stage events on >= 8 steps of the region, never on the priming step
                timer.active = sampled_step(it, steps) if not args.timer_every else (it > 0 and it % args.timer_every == 0)
                timer.sampled_steps += int(timer.active)
                timer.mark("begin")

        def after_step(it):
            if timer:
                timer.mark("mlp_glue")
            ring[it % run_ahead].record()

        if pipelined:
            # N > 1 (or the one-rank rehearsal): the library's own sharded scoring loop — two batches in flight, every
            # rank keeps its slices, ONE all-gather closes the loop inside the timed region
            from ocn_amd.pipeline import pipelined_shard_loop
            with torch.no_grad():
                scores, pattern[0] = pipelined_shard_loop(begin, finish, steps, B_total,
                                                          gather_at_end=True, before_step=before_step, after_step=after_step,
                                                          overlap=overlap)
            out = scores[-1]
            if world == 1 and not args.rehearse_collectives:
                pattern[0] = "single rank: no collective; " + pattern[0]
        else:
            for it in range(steps):
                before_step(it)
                out = step(it, last=(it == steps - 1))
                after_step(it)
        t_wait = t_waits[0]
        t_launch = time.perf_counter() - t0 - t_wait    # host time spent enqueueing (flow-control waits excluded)
        if pending[0] is not None:
            pending[0].wait()
            pending[0] = None
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        gc.enable()
        ops.stage_timer = None
        if world > 1:
            tmax = torch.tensor([dt], device=dev, dtype=torch.float64)
            dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
            dt = tmax.item()
        return dt, t_launch, out

    if not args.full:
        args.no_stage_timers = True                # (a plain run: the headline loop only, no stage events in it)
    timer = None if args.no_stage_timers else StageTimer(pool=48 * (args.steps // max(args.timer_every or max(1, args.steps // 8), 1) + 2), lean=not args.all_stages)
    dt, t_launch, out = timed_loop(args.steps, timer)
    pattern_main = pattern[0]
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, out)
    if not args.full:
        args.repeats, args.no_validate_leg, args.no_cpu_baseline = 1, True, True
    # the same timed loop again (no stage events): the spread of the step time from run to run, reported beside `value`
    runs = [dt / args.steps] + [timed_loop(args.steps, None)[0] / args.steps for _ in range(max(args.repeats, 1) - 1)]
    pattern[0] = pattern_main
    # The same loop on ONE stream (untimed for `value`): per-kernel durations without the other stream's kernels beside
    # them — under the two-stream overlap a launch's duration includes what it yields to its neighbour — and the step time
    # the overlap is measured against.  Reported next to the timed region's own figures, never instead of them.
    timer1, dt1 = None, None
    overlapped = pipelined and "HIP stream" in pattern_main
    if overlapped and not args.no_stage_timers and not args.no_one_stream_leg:
        n1 = min(args.steps, 64)
        timer1 = StageTimer(pool=48 * (n1 // max(args.timer_every or max(1, n1 // 8), 1) + 2), lean=not args.all_stages)
        dt1, _, _ = timed_loop(n1, timer1, overlap=False)
        dt1 /= n1
        pattern[0] = pattern_main
    # second leg: the per-batch id check left on (the drivers' literal loop: one host sync per batch)
    dt_val = None
    if not args.no_validate_leg and not args.graph:
        graphed[0] = None                          # (the per-batch id check is a host sync inside begin(): launch by launch)
        ops.validate_indices = True
        for i in range(4):
            step(i)
        dt_val, _, _ = timed_loop(min(args.steps, 64), None)
        dt_val /= min(args.steps, 64)
        ops.validate_indices = False

    # third leg (cn5 only, fresh model in the main leg): the same loop with a TRAINED checkpoint's innerprod buffer — the
    # second column normalisation is then summed in the reference's entry order (ocn_cn_colsum_exact), which every real
    # inference checkpoint pays; VERDICT r2 asked for this figure in the default line
    dt_tr, err_tr = None, None
    if cfg["pred"] == "cn5" and not args.innerprod and not args.graph and not args.no_validate_leg:
        with torch.no_grad():
            pred.innerprod.fill_(0.37)
        for i in range(4):
            step(i)
        new_graphs()
        if graphed[0] is not None:                 # (two eager uses and the capture of every scratch set, untimed)
            from ocn_amd.pipeline import pipelined_shard_loop
            with torch.no_grad():
                pipelined_shard_loop(begin, finish, 4 * graphed[0].n_sets, B_total, gather_at_end=True)
        n_tr = min(args.steps, 64)
        dt_tr, _, _ = timed_loop(n_tr, None)
        dt_tr /= n_tr
        with torch.no_grad():
            pred.innerprod.fill_(0.0)
        graphed[0] = None                          # (step() finishes launch by launch)
        step(0)

    if rank == 0:
        idx = {"cora": 0, "collab": 1, "ppa": 2, "citation2": 3, "ddi": 4}[args.dataset]
        line = {
            "metric": f"candidate-edges/sec (CN predictor fwd), ogbl-{args.dataset} shape",
            "value": B_total * args.steps / dt, "unit": "edges/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True,
            "scaling": args.scaling, "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "dtype_detail": ("sparse stage (intersection, column weights, pooling): f32 products and sums rounded separately, "
                             "integer counts exact; MLP heads: "
                             + ("f16x3-split, f32 accumulate (each f32 product = three f16 MFMAs on hi/lo splits of both operands; the "
                                "dropped lo*lo term is below 2^-22 relative)" if H >= ops.fused_heads_min_width and ops.fused_heads
                                else "bf16x6-split, f32 accumulate (each f32 product = six bf16 MFMAs)")),
            "config": {"workload": f"ogbl-{args.dataset}-shaped synthetic graph, {cfg['enc']} {cfg['conv']} x{cfg['layers']} "
                                   f"hiddim={H} predictor={cfg['pred']} built as the reference drivers build it (only cndeg "
                                   f"forwarded: tailact=False, use_xlin=False, beta=1, lnnn={cfg['lnnn']}; head = "
                                   f"{head_layout(pred)}), CN route={cfg['route']}, "
                                   + (f"batch {cfg['batch']} per GPU, " if args.scaling == "weak" else
                                      f"ONE batch of {cfg['batch']} candidates cut over the {world} GPUs ({B_total // world} per GPU: strong scaling), ")
                                   + f"{NB} distinct seeded batches in rotation, ids bounds-checked once before the timed "
                                   f"region (BASELINE.json configs[{idx}])",
                       "nodes": wl["n"], "nnz": wl["nnz"], "nnz_A2": wl["nnz2"], "max_deg": wl["max_deg"],
                       "global_batch": B_total, "parallelism": f"edge-shard x{world}", "graph_scale": args.scale,
                       "batches_in_rotation": NB, "innerprod": args.innerprod},
            "host_enqueue_ms_per_step": t_launch / args.steps * 1e3,
            "communication_pattern": pattern[0],
            "score_checksum": float(out.double().sum().item()),
        }
        if args.full:
            per = [batch_bytes(wl, m, H) for m in mines]
            ab = {k: sum(p[k] for p in per) / NB for k in per[0]}
            stages = {k: dict(ms=v[0], launches=v[1], ms_per_step=v[2]) for k, v in (timer.totals() if timer else {}).items()}
            sampled = max(timer.sampled_steps, 1) if timer else 1
            roof, roof_hbm, roofs = None, None, {}
            if stages:
                kname = {"cn_flags": "cn_walk_kernel" if cfg["route"] == "walk" else "cn_flags_kernel",
                         "cn_gather": "cn_gather_wave_kernel" if (H <= 64 and mines[0].shape[1] * (H // 4) < 262144) else "cn_gather_kernel"}
                for k, comp, form in (("cn_flags", "flags_compulsory", "flags_formula"), ("cn_gather", "gather_compulsory", "gather_formula")):
                    if k not in stages:
                        continue
                    t = stages[k]["ms"] * 1e-3
                    tr = pmc(kname[k])
                    roofs[k] = dict(bound="hbm", kernel=kname[k], achieved=ab[comp] / t / 1e9, peak=HBM_PEAK / 1e9, unit="GB/s",
                                    frac=ab[comp] / t / HBM_PEAK, traffic=tr,
                                    traffic_frac=None if tr is None else tr / t / HBM_PEAK,
                                    algorithmic_bytes_per_launch=ab[comp], survey_formula_bytes_per_launch=ab[form],
                                    survey_formula_GBps=ab[form] / t / 1e9, avg_launch_ms=stages[k]["ms"],
                                    note="achieved = compulsory bytes of the batch (distinct embedding / weight rows once, "
                                         "CSR rows walked, outputs) / launch time; the SURVEY §8d formula (one row per CN "
                                         "entry, whole A² row) is printed beside it and may exceed the HBM peak because "
                                         "shared rows are served by L2; traffic = PMC 2*FETCH_SIZE + WRITE_SIZE of the "
                                         "committed profile")
                    stages[k]["compulsory_GBps"] = roofs[k]["achieved"]
                stages1 = {k: dict(ms=v[0], launches=v[1], ms_per_step=v[2]) for k, v in (timer1.totals() if timer1 else {}).items()}
                # the dominant kernel: the stage with the most time per STEP inside the timed region (same-stream event pairs)
                dom = max((k for k in ("cn_flags", "cn_gather", "linear") if k in stages), key=lambda k: stages[k]["ms_per_step"])
                roof_hbm = roofs.get("cn_gather")
                if "linear" in stages:
                    # MFMA work of the MLP heads per launch.  The fused kernel (ocn_heads_fused, H >= 128) multiplies a row by
                    # 8 H x H panels (the reference's 9 Linear(H,H): the last layer of each branch is folded into lin's Linear
                    # offline, model._fused_pack), skips, per 128-row tile of the class-major order, the pooled branches whose
                    # input is all zero, and evaluates every f32 product as THREE f16 MFMAs (hi/lo splits of both operands).
                    # The grouped Linear launches (narrower heads) issue six bf16 MFMAs per product.  frac is the fraction of
                    # the pipe the kernel runs on: issued f16 / bf16 MFMA FLOPs over the dense 16-bit MFMA peak.
                    launches_per_step = stages["linear"]["launches"] / sampled
                    Bm = mines[0].shape[1]
                    t = stages["linear"]["ms"] * 1e-3
                    fused = bool(ops.fused_heads and H >= ops.fused_heads_min_width and getattr(pred, "_fused_plan", lambda H: None)(H) is not None)
                    ref_fl = timer.flops.get("linear", 0.0) / stages["linear"]["launches"]
                    skip = getattr(pred, "_skip_state", None)
                    skipping = bool(ops.skip_zero_rows and skip is not None and skip["off"] == 0 and Bm >= ops.skip_zero_min_batch)
                    n_cn1, n_any = ab["n_cn1"], ab["n_any"]
                    n_b = n_any if pred._xcn2_on_union else ab["n_cn2"]
                    if fused:
                        rows_a, rows_b = (n_cn1, n_b) if skipping else (Bm, Bm)
                        f32_fl = 2.0 * H * H * (3 * rows_a + 3 * rows_b + 2 * Bm) / launches_per_step
                        kern, terms, pipe = "heads_fused_kernel", 3, "f16"
                    else:
                        f32_fl = ref_fl
                        if skipping and pred._heads_plan(H) is not None:
                            sx_layers = len(pred._heads_plan(H)[2])
                            lin_layers = sum(1 for m in pred.lin if isinstance(m, torch.nn.Linear) and m.out_features == H)
                            f32_fl = (2.0 * H * H * (2 * n_cn1 + 2 * n_b + sx_layers * Bm + lin_layers * Bm)
                                      + 2.0 * (2 * H) * H * n_any) / launches_per_step
                        kern, terms, pipe = "linear_bf16x6_kernel", 6, "bf16"
                    issued = terms * f32_fl
                    roofs["heads"] = dict(bound="mfma", kernel=kern, achieved=issued / t / 1e12, peak=BF16_MFMA_PEAK / 1e12,
                                          unit="TFLOP/s", frac=issued / t / BF16_MFMA_PEAK, traffic=pmc(kern),
                                          algorithmic_flops_per_launch=issued, avg_launch_ms=stages["linear"]["ms"],
                                          launches_per_step=launches_per_step, mfma_per_f32_product=terms, mfma_dtype=pipe,
                                          f32_equivalent_tflops=f32_fl / t / 1e12, f32_equivalent_flops_per_launch=f32_fl,
                                          f32_equivalent_frac_of_f32_mfma_peak=f32_fl / t / F32_MFMA_PEAK,
                                          reference_head_f32_flops_per_step=2.0 * H * H * 9 * Bm + 2.0 * H * Bm,
                                          skipped_zero_rows=skipping,
                                          note=f"achieved / peak / frac = the {pipe} MFMA FLOPs the launch issues ({terms} MFMAs per f32 "
                                               "product; 2*H*H per row and panel, rows of skipped all-zero branches excluded, the 9 "
                                               "Linear(H,H) of the reference folded to 8 panels) against the dense 16-bit MFMA peak; "
                                               "f32_equivalent_* = the same work counted once per f32 product.  MFMA-busy counters: "
                                               "profiles/r03_heads_pmc.json.  Head: " + head_layout(pred))
                for k, rk in (("cn_flags", "cn_flags"), ("cn_gather", "cn_gather"), ("linear", "heads")):
                    if rk in roofs and k in stages1:
                        t1 = stages1[k]["ms"]
                        roofs[rk]["avg_launch_ms_one_stream"] = t1
                        roofs[rk]["frac_one_stream"] = roofs[rk]["frac"] * roofs[rk]["avg_launch_ms"] / t1
                        stages[k]["ms_one_stream"] = t1
                        roofs[rk]["note"] += ("  avg_launch_ms / achieved / frac are measured inside the timed region, where the intersection pass "
                                              "of the next batch runs on a second stream beside this kernel; *_one_stream = the same launch "
                                              "with the streams serialised.")
                roof = roofs["heads"] if dom == "linear" else roofs[dom]
            cpu, err, ref_scale = None, None, None
            if world == 1 and not args.no_cpu_baseline:
                cpu, b, ref = cpu_baseline(wl, args, mines[0])
                ops.validate_indices = False
                sub = mines[0][:, :b].contiguous()
                with torch.no_grad():
                    c1, c2 = cn_handles(wl, sub)
                    got = pred(h, adj, c1, c2, sub, wl["args"]).cpu()
                err = (got - ref).abs().max().item()
                ref_scale = ref.abs().max().item()
            line["config"].update({
                "mean_deg_src": ab["mean_di"], "mean_deg_dst": ab["mean_dj"],
                "mean_second_operand_len": ab["mean_second"],
                "mean_cn1": ab["mean_c1"], "mean_cn2": ab["mean_c2"],
                "distinct_h_rows_per_batch": ab["distinct_h_rows"],
                "frac_rows_with_cn1": ab["frac_rows_cn1"], "frac_rows_with_any_cn": ab["frac_rows_any"]})
            line.update({
                "value_runs": [B_total / r for r in runs], "value_min": B_total / max(runs),
                "value_median": B_total / sorted(runs)[len(runs) // 2], "ms_per_step_runs": [r * 1e3 for r in runs],
                "stage_timer": {"sampled_steps": sampled, "rule": "HIP events on the launch stream, same-stream pairs only, "
                                ">= 8 sampled steps, never the priming step"},
                "roofline": roof, "roofline_hbm_kernel": roof_hbm, "rooflines": roofs, "cpu_baseline": cpu,
                "value_trained_innerprod": None if dt_tr is None else B_total / dt_tr,
                "ms_per_step_trained_innerprod": None if dt_tr is None else dt_tr * 1e3,
                "value_one_stream": None if dt1 is None else B_total / dt1,
                "ms_per_step_one_stream": None if dt1 is None else dt1 * 1e3,
                "value_validate_per_batch": None if dt_val is None else B_total / dt_val,
                "ms_per_step_validate_per_batch": None if dt_val is None else dt_val * 1e3,
                "stages": stages,
                "once_per_graph": {"encoder_ms": wl["enc_s"] * 1e3, "adj2_build_ms": wl["a2_s"] * 1e3,
                                   "graph_build_s": wl["graph_s"]},
                "algorithmic_bytes_per_step": ab["flags_compulsory"] + ab["gather_compulsory"],
                "survey_formula_bytes_per_step": ab["flags_formula"] + ab["gather_formula"],
                "parity_on_cpu_sample_max_abs_err": err,
                "parity_on_cpu_sample_max_abs_ref": ref_scale,         # the scores' scale: raw walk-count pools (citation2) reach 1e4
                "parity_on_cpu_sample_rel_err": None if not ref_scale else err / ref_scale,
            })
        print(json.dumps(line), flush=True)
    if world > 1:
        dist.barrier()
    if dist.is_initialized():
        dist.destroy_process_group()


if __name__ == "__main__":
    try:
        main()
    finally:                                       # the timed loops switch the per-batch id check off: never leave it off
        from ocn_amd import ops as _ops
        _ops.validate_indices = True
