"""The reference's training / evaluation driver (NeighborOverlap_large.py: train() :28-94, test()
:97-180, the epoch loop of main() :300-345) written against ocn_amd, on a synthetic dataset of the
named shape (no network: ogb / Planetoid downloads are replaced by ocn_amd.synth.loaddataset_like,
ogb's Evaluator by ocn_amd.evaluate.Evaluator).  Everything between the import block and the
argument parser is the reference's call sequence with the three import lines swapped
(INTEGRATION.md §2).

    python examples/run_like_reference.py --dataset cora --predictor cn5 --epochs 5
    python examples/run_like_reference.py --dataset collab --scale 0.05 --hiddim 64 --batch_size 8192
    python examples/run_like_reference.py --dataset citeseer --model puremean --mplayers 3 --nnlayers 1 --hiddim 64 \
        --gnnedp 0.07 --res --maskinput --batch_size 384
    python examples/run_like_reference.py --dataset cora --epochs 5 --table-dtype bf16    # test() and --recommend pool from a bf16 table of h
    python examples/run_like_reference.py --dataset cora --epochs 5 --table-dtype int8 --cn-cap 32    # ... from int8 rows, capped
    python examples/run_like_reference.py --dataset cora --epochs 5 --cn-cap 8:1          # ... pooling at most 8 sampled common neighbours per candidate (seed 1)
    python examples/run_like_reference.py --dataset cora --heuristic ra        # no training: a classical baseline's metric
    python examples/run_like_reference.py --dataset cora --heuristic ra --recommend 5     # ... and its top-5 targets per source
    python examples/run_like_reference.py --dataset cora --recommend 5 --recommend-walk   # top-5 of the model without forming A²
    python examples/run_like_reference.py --dataset cora --recommend 5 --recommend-frozen # ... with column weights frozen on the validation edges
    python examples/run_like_reference.py --dataset cora --recommend 5 --recommend-frozen --recommend-prefilter ra:32   # ... ranking a short list only
    python examples/run_like_reference.py --dataset cora --recommend 5 --recommend-hops 3 --recommend-frozen --recommend-prefilter ra:32:0.5   # ... over 3 hops
    python examples/run_like_reference.py --dataset cora --recommend 5 --recommend-frozen --recommend-prefilter ra:32 --recommend-eval 200   # ... and where the test links rank
    python examples/run_like_reference.py --dataset cora --recommend 5 --recommend-frozen --recommend-long ra:300 --recommend-eval 200   # ... a short list beyond 128
    python examples/run_like_reference.py --dataset cora --recommend 5 --recommend-rw 32:256:2 --recommend-eval 200   # ... a short list from random walks instead
    python examples/run_like_reference.py --dataset cora --recommend 5 --recommend-emb 32 --recommend-eval 200        # ... the nearest embeddings over ALL nodes instead
    python examples/run_like_reference.py --dataset cora --recommend 5 --recommend-prefilter ra:32 --recommend-emb 32:cos --recommend-union --recommend-eval 200   # ... or the union of the two
    python examples/run_like_reference.py --dataset cora --recommend 5 --recommend-frozen --recommend-explain 3       # ... and why: each link's top-3 common neighbours
    python examples/run_like_reference.py --dataset cora --recommend 5 --recommend-frozen --recommend-explain-edges 10 # ... down to the edges: the 10 strongest messages
    python examples/run_like_reference.py --dataset cora --heuristic ra --recommend 5 --recommend-accept 3 --recommend-undo
    python examples/run_like_reference.py --dataset cora --structured-negatives           # training negatives that are never links
    python examples/run_like_reference.py --dataset citation2 --scale 0.002 --hiddim 64 --structured-negatives   # ... and MRR negatives
    python examples/run_like_reference.py --dataset cora --hard-negatives 0.5              # half the training negatives from the source's 2-hop candidates
    python examples/run_like_reference.py --dataset citation2 --scale 0.002 --hiddim 64 --hard-negatives 0.5 --hard-eval-negatives   # ... and MRR negatives
"""
import argparse
import math
import os
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ocn_amd import ops                                                             # noqa: E402
from ocn_amd.evaluate import Evaluator                                              # noqa: E402
from ocn_amd.explain import explain_link_edges, explain_links                       # noqa: E402
from ocn_amd.frozen import freeze_columns                                           # noqa: E402
from ocn_amd.heuristics import KINDS, TWO_HOP, score_edges_heuristic                # noqa: E402
from ocn_amd.model import GCN, predictor_dict                                       # noqa: E402
from ocn_amd.pipeline import embedding_table, embedding_table_int8, score_mrr_split  # noqa: E402
from ocn_amd.ranking import rank_links, rank_links_heuristic, ranking_metrics       # noqa: E402
from ocn_amd.recommend import (EmbeddingNeighbours, RandomWalks, ShortListUnion, random_walk_short_list, prefilter_candidates, recommend_links, recommend_links_heuristic,  # noqa: E402
                               three_hop_candidates, two_hop_candidates, PathSums, prefilter_candidates_long)
from ocn_amd.update import EncoderState, insert_edges, remove_edges                 # noqa: E402
from ocn_amd.sampling import (negative_edges, negative_targets, two_hop_negative_edges,  # noqa: E402
                              two_hop_negative_targets)
from ocn_amd.sparse import SparseTensor                                             # noqa: E402
from ocn_amd.synth import loaddataset_like                                          # noqa: E402
from ocn_amd.utils import PermIterator, adjoverlap, sparse_tensor_multiply          # noqa: E402


def build_adj2(adj, args):
    if args.adj2byblock:
        return sparse_tensor_multiply(SparseTensor.from_torch_sparse_coo_tensor(adj.to_torch_sparse_coo_tensor()), 1024)
    spadj = adj.to_torch_sparse_coo_tensor()
    return SparseTensor.from_torch_sparse_coo_tensor(spadj @ spadj, False)


def train(model, predictor, data, split_edge, optimizer, batch_size, maskinput, args, epoch=0):
    model.train(); predictor.train()
    pos_train_edge = split_edge['train']['edge'].to(data.x.device).t()
    total_loss = []
    adjmask = torch.ones_like(pos_train_edge[0], dtype=torch.bool)
    if args.structured_negatives:
        # non-edges only, as the reference's negative_sampling call returns them (NeighborOverlap_large.py:51); one draw per epoch
        negedge = negative_edges(data.adj_t, pos_train_edge.shape[1], seed=epoch)
    else:
        negedge = torch.randint(0, data.num_nodes, pos_train_edge.shape, device=pos_train_edge.device)
    share = round(100 * args.hard_negatives)
    if share:
        # positive t with t % 100 < share gets its target corrupted within the source's 2-hop candidates (the pairs that
        # recommend_links / rank_links order) in place of the draw above; a source without a candidate keeps that draw.
        # PermIterator shuffles, so every batch gets the mix.  One draw per epoch.
        t = torch.arange(pos_train_edge.shape[1], device=pos_train_edge.device)
        t = t[t % 100 < share]
        hard = two_hop_negative_edges(data.adj_t, pos_train_edge[:, t], seed=epoch, fallback=None)
        negedge[:, t] = torch.where(hard[1] >= 0, hard, negedge[:, t])
    for perm in PermIterator(adjmask.device, adjmask.shape[0], batch_size):
        optimizer.zero_grad()
        if maskinput:
            adjmask[perm] = 0
            tei = pos_train_edge[:, adjmask]
            adj = SparseTensor.from_edge_index(tei, sparse_sizes=(data.num_nodes, data.num_nodes)).to_device(
                pos_train_edge.device, non_blocking=True)
            adjmask[perm] = 1
            adj = adj.to_symmetric()
        else:
            adj = data.adj_t
        h = model(data.x, adj)
        adj2 = build_adj2(adj, args)
        edge = pos_train_edge[:, perm]
        pos_outs = predictor.multidomainforward(h, adj, adjoverlap(adj, adj, edge), adjoverlap(adj, adj2, edge), edge,
                                                args, cndropprobs=[])
        pos_losss = -F.logsigmoid(pos_outs).mean()
        edge = negedge[:, perm]
        neg_outs = predictor.multidomainforward(h, adj, adjoverlap(adj, adj, edge), adjoverlap(adj, adj2, edge), edge,
                                                args, cndropprobs=[])
        neg_losss = -F.logsigmoid(-neg_outs).mean()
        loss = neg_losss + pos_losss
        loss.backward()
        optimizer.step()
        total_loss.append(loss.detach())
    return float(torch.stack(total_loss).mean())


def _table(h, dtype):
    """--table-dtype: ``h`` as the table the predictor pools from (pipeline.embedding_table; "int8": embedding_table_int8)."""
    return embedding_table_int8(h) if dtype == "int8" else embedding_table(h, dtype)


@torch.no_grad()
def test(model, predictor, data, split_edge, evaluator, batch_size, use_valedges_as_input, args):
    model.eval(); predictor.eval()
    dev = data.x.device
    edges = {k: split_edge[s][f].to(dev) for k, (s, f) in dict(
        pos_train=('train', 'edge'), pos_valid=('valid', 'edge'), neg_valid=('valid', 'edge_neg'),
        pos_test=('test', 'edge'), neg_test=('test', 'edge_neg')).items()}
    adj = data.adj_t
    h = model(data.x, adj)
    adj2 = build_adj2(adj, args)
    table = lambda h: _table(h, args.table_dtype)        # --table-dtype: cast once per embedding matrix, never per batch

    def score(e, h, adj):
        return torch.cat([predictor(h, adj, adjoverlap(adj, adj, e[perm].t()), adjoverlap(adj, adj2, e[perm].t()),
                                    e[perm].t(), args).squeeze(-1)
                          for perm in PermIterator(e.device, e.shape[0], batch_size, False)], dim=0)

    t = table(h)
    pred = {k: score(edges[k], t, adj) for k in ("pos_train", "pos_valid", "neg_valid")}
    if use_valedges_as_input:
        adj = data.full_adj_t
        h = model(data.x, adj)
        t = table(h)
    pred.update({k: score(edges[k], t, adj) for k in ("pos_test", "neg_test")})
    results = {}
    for K in [20, 50, 100]:
        evaluator.K = K
        hits = [evaluator.eval({'y_pred_pos': pred[p], 'y_pred_neg': pred[n]})[f'hits@{K}']
                for p, n in (("pos_train", "neg_valid"), ("pos_valid", "neg_valid"), ("pos_test", "neg_test"))]
        results[f'Hits@{K}'] = tuple(hits)
    return results, h


@torch.no_grad()
def test_mrr(model, predictor, data, split_edge, evaluator, batch_size, use_valedges_as_input, args):
    """The citation2 evaluation (NeighborOverlapCitation2.py:227-254): per positive (source, target) the negatives that share
    its source, scored on the walk route by ``pipeline.score_mrr_split``; the mean reciprocal rank of valid and test.  The
    negatives are the split's own (uniform random targets), or with --structured-negatives as many per source from
    ``negative_targets(data.full_adj_t, ..)``: never the source itself and never a link the model has seen.  With
    --hard-eval-negatives they come from ``two_hop_negative_targets(data.full_adj_t, ..)`` instead: non-links within two hops
    of the source, the pairs a recommendation has to order (uniform non-links where a source has no such node)."""
    model.eval(); predictor.eval()
    dev = data.x.device
    out = []
    for seed, (split, adj) in enumerate((("valid", data.adj_t), ("test", data.full_adj_t if use_valedges_as_input else data.adj_t))):
        source = split_edge[split]['edge'][:, 0].to(dev).contiguous()
        target = split_edge[split]['edge'][:, 1].to(dev).contiguous()
        neg = split_edge[split]['edge_neg'][..., 1].to(dev).contiguous()
        if args.hard_eval_negatives:
            neg = two_hop_negative_targets(data.full_adj_t, source, neg.shape[1], seed=seed)
        elif args.structured_negatives:
            neg = negative_targets(data.full_adj_t, source, neg.shape[1], seed=seed)
        out.append(score_mrr_split(predictor, _table(model(data.x, adj), args.table_dtype), adj, source, target, neg, batch_size, args, evaluator))
    return {'MRR': tuple(out)}, None


@torch.no_grad()
def test_heuristic(kind, data, split_edge, evaluator, batch_size, args):
    """The dataset's metric for one training-free heuristic (ocn_amd.heuristics) on valid and test: the scores of test()
    with the encoder and the predictor left out.  Test candidates see the validation edges with --use_valedges_as_input."""
    dev = data.x.device
    out = {}
    for split, adj in (("valid", data.adj_t), ("test", data.full_adj_t)):
        adj2 = build_adj2(adj, args) if kind in TWO_HOP else None
        pos = score_edges_heuristic(adj, adj2, split_edge[split]['edge'].to(dev), batch_size, kind)
        neg = score_edges_heuristic(adj, adj2, split_edge[split]['edge_neg'].to(dev), batch_size, kind)
        out[split] = evaluator.eval({'y_pred_pos': pos, 'y_pred_neg': neg})[evaluator.eval_metric]
    return out


def rw_name(rw):
    return f"random walks {rw.m}:{rw.walks}:{rw.length}" + (f":{rw.decay:g}" if rw.decay is not None else "")


def prefilter_name(pf):
    if isinstance(pf, RandomWalks):
        return rw_name(pf)
    if isinstance(pf, EmbeddingNeighbours):
        return f"embedding {pf.m}" + (":cos" if pf.normalize else "")
    if isinstance(pf, ShortListUnion):
        return "union of " + " + ".join(prefilter_name(st) for st in pf.stages)
    if isinstance(pf, PathSums):
        return f"long {pf.kind}:{pf.m}" + (f":{pf.decay:g}" if pf.decay is not None else "")
    return ":".join(f"{p:g}" if isinstance(p, float) else str(p) for p in pf)


@torch.no_grad()
def recommend(k, data, split_edge, args, model=None, predictor=None, n_sources=5):
    """--recommend K: the K best predicted new links of the first few test sources (ocn_amd.recommend), by the heuristic or by
    the trained model, on the adjacency that test candidates see; a source with fewer than K candidates is padded with -1.
    --recommend-walk: without A² — candidates expanded from the adjacency, the model's scores on the walk route.
    --recommend-frozen: cn5 / cn7 score with column weights frozen on the validation positives; a call for half the sources
    is checked to return the same rows.
    --recommend-prefilter KIND:M: the model ranks only the M best candidates of every source by the heuristic KIND (cn, aa, ra);
    with --recommend-frozen the number of unfiltered top-K links that the short list kept is printed.
    --recommend-hops 3: the candidates within three hops (every target with a non-empty cn1 or cn2), expanded from the adjacency;
    the prefilter is then KIND:M:DECAY and ranks them by the local path index P2 + DECAY * P3.
    --recommend-long KIND:M[:DECAY]: the same short list for ANY M >= K (ocn_amd.recommend.PathSums: the M best taken as a set by
    ocn_segment_keep_best, no limit of 128); --recommend-prefilter keeps its limit and its route.
    --recommend-rw M:W:L[:DECAY]: the short list comes from W random walks of L steps per source instead (the M most visited nodes,
    ranked by c2 + DECAY * c3; ocn_amd.recommend.RandomWalks): a sample of the candidates at a cost that no hub source raises.
    --recommend-emb M[:cos]: the short list is the M nodes nearest to the source's embedding by int8 inner product (cosine with
    :cos), over ALL nodes (ocn_amd.recommend.EmbeddingNeighbours): a source without neighbours gets targets too.
    --recommend-union: beside --recommend-prefilter or --recommend-rw, the model ranks the union of that short list and the
    --recommend-emb one (ocn_amd.recommend.ShortListUnion).
    --recommend-eval Q: the held-out test links of the first Q distinct test sources are ranked among the candidates of the selected
    route (ocn_amd.ranking) and recall / NDCG / hit rate @K, MRR, coverage and retention are printed; with a prefilter the
    unfiltered run stands beside it.
    --recommend-explain M: the K winners of the printed sources are explained as ONE batch (ocn_amd.explain): per target the M
    common neighbours that carry most of its score, with their two shares (via xcn1, via xcn2).
    --recommend-accept M: the M best of them are then inserted and the sources asked again.
    --recommend-undo: the accepted links are then removed again, and the restored pair is compared with the original.
    --recommend-check-refresh: the refreshed node embeddings are compared with a full encoder pass after either update."""
    dev = data.x.device
    adj = data.full_adj_t
    adj2 = None if args.recommend_walk else build_adj2(adj, args)
    sources = split_edge['test']['edge'][:n_sources, 0].to(dev).contiguous()

    state = None
    if not args.heuristic:
        model.eval(); predictor.eval()
        if args.recommend_accept > 0:
            state = EncoderState(model, data.x, adj)      # h and its per-layer activations stay resident beside A and A²

    def table(adj):
        # --table-dtype: the embeddings the model requests pool from, cast once per request (pipeline.embedding_table)
        return _table(state.h if state is not None else model(data.x, adj), args.table_dtype)

    def refreshed(adj, edges, tag):
        rows = state.refresh(adj, edges)                  # only the rows the update can reach are recomputed
        print(f"refreshed {rows.numel()} of {state.n} embedding rows after {tag} ({state.route} route)", flush=True)
        if args.recommend_check_refresh and not torch.equal(state.h, model(data.x, adj)):
            raise SystemExit(f"--recommend-check-refresh: the refreshed embeddings differ from a full pass after {tag}")

    def top(adj, adj2, tag):
        if args.heuristic:
            dst, score = recommend_links_heuristic(adj, adj2, sources, k, args.testbs, args.heuristic, hops=args.recommend_hops)
        else:
            h = table(adj)
            dst, score = recommend_links(predictor, h, adj, adj2, sources, k, args.testbs, args, prefilter=args.recommend_prefilter,
                                         hops=args.recommend_hops)
        for s, d, v in zip(sources.tolist(), dst.tolist(), score.tolist()):
            print(f"{tag} source {s} top-{k}: " + " ".join(str(t) for t in d) + "  scores: " + " ".join(f"{x:.4f}" for x in v),
                  flush=True)
        return dst, score

    if args.recommend_frozen:
        # --recommend-frozen: the column weights of cn5 / cn7 are taken once, from the validation positives as ONE reference batch
        # (ocn_amd.frozen), and kept: a candidate's score then depends on nobody else who is asked about
        ref = split_edge['valid']['edge'].to(dev)[:ops.MAX_BATCH].contiguous()
        fc = freeze_columns(predictor, adj, adj2, ref, args)
        predictor.set_frozen_columns(fc, args)
        print(f"frozen {fc.kind} column weights from {fc.ref_size} validation edges ({'walk' if fc.valued else 'pattern'} route)", flush=True)

    dst, score = top(adj, adj2, "recommend")
    if args.recommend_frozen:
        h = table(adj)
        _, half = recommend_links(predictor, h, adj, adj2, sources[::2].contiguous(), k, max(args.testbs // 3, 1), args,
                                  prefilter=args.recommend_prefilter, hops=args.recommend_hops)    # (like with like: a source's short list is its own)
        same = torch.allclose(half, score[::2], rtol=1e-5, atol=1e-5)
        print(f"a call for every second source at a third of the batch size returns the same rows = {same}", flush=True)
        if not same:
            raise SystemExit("--recommend-frozen: the scores of a source changed with the other sources of the call")
        if args.recommend_prefilter:
            # how many of the unfiltered top-K the short list kept: printed only — a synthetic graph under an untrained or briefly
            # trained model supports no claim about the quality of a prefilter
            full, _ = recommend_links(predictor, h, adj, adj2, sources, k, args.testbs, args, hops=args.recommend_hops)
            kept = int(((dst[:, :, None] == full[:, None, :]) & (full[:, None, :] >= 0)).any(1).sum())
            if isinstance(args.recommend_prefilter, (EmbeddingNeighbours, ShortListUnion)):
                n_all = n_short = None                       # (an embedding list is not a subset of the candidates within the hops)
                name = prefilter_name(args.recommend_prefilter)
            elif isinstance(args.recommend_prefilter, RandomWalks):
                n_all = int((three_hop_candidates(adj, sources) if args.recommend_hops == 3 else two_hop_candidates(adj, adj2, sources))[0][-1])
                n_short = int(random_walk_short_list(adj, sources, args.recommend_prefilter)[0][-1])
                name = rw_name(args.recommend_prefilter)
            elif isinstance(args.recommend_prefilter, PathSums):
                n_all = int((three_hop_candidates(adj, sources) if args.recommend_hops == 3 else two_hop_candidates(adj, adj2, sources))[0][-1])
                n_short = int(prefilter_candidates_long(adj, sources, args.recommend_prefilter, hops=args.recommend_hops)[0][-1])
                name = prefilter_name(args.recommend_prefilter) + (" over 3 hops" if args.recommend_hops == 3 else "")
            elif args.recommend_hops == 3:
                kind, m, decay = args.recommend_prefilter
                n_all = int(three_hop_candidates(adj, sources)[0][-1])
                n_short = int(prefilter_candidates(adj, sources, kind, m, hops=3, decay=decay)[0][-1])
                name = f"{kind}:{m}:{decay:g} over 3 hops"
            else:
                kind, m = args.recommend_prefilter
                n_all = int(two_hop_candidates(adj, adj2, sources)[0][-1])
                n_short = int(prefilter_candidates(adj, sources, kind, m)[0][-1])
                name = f"{kind}:{m}"
            print(f"prefilter {name} kept {kept} of the {int((full >= 0).sum())} unfiltered top-{k} links"
                  + (f" (the model ranked {n_short} of {n_all} candidates)" if n_all is not None else ""), flush=True)
    if args.recommend_eval:
        # --recommend-eval Q: where the held-out test links land in the ranking served above (ocn_amd.ranking).  The first Q distinct
        # test sources; truth = the test edges, both ways, on the graph the candidates come from.  Printed only: a synthetic graph
        # under a briefly trained model supports no claim about which route ranks best.
        test = split_edge['test']['edge'].to(dev)
        n = adj.size(0)
        first = torch.tensor(list(dict.fromkeys(test[:, 0].tolist()))[:args.recommend_eval], dtype=torch.int64, device=dev)
        truth = SparseTensor.from_edge_index(test.t().contiguous(), sparse_sizes=(n, n)).to_symmetric()
        ks = tuple(sorted({k, 10, 50, 100}))

        def show(tag, res):
            met = ranking_metrics(res, ks)
            print(f"recommend-eval {tag}: {met['n_eval']} sources, {met['n_pairs']} pairs, coverage {met['coverage']:.4f}"
                  + (f" retention {met['retention']:.4f}" if "retention" in met else "") + f" mrr {met['mrr']:.4f}  "
                  + "  ".join(f"recall/ndcg/hit@{x} {met[f'recall@{x}']:.4f}/{met[f'ndcg@{x}']:.4f}/{met[f'hit_rate@{x}']:.4f}" for x in ks),
                  flush=True)
        if args.heuristic:
            show(f"{args.heuristic} over {args.recommend_hops} hops",
                 rank_links_heuristic(adj, adj2, first, truth, args.testbs, args.heuristic, hops=args.recommend_hops))
        else:
            h = table(adj)
            route = f"{args.predictor} over {args.recommend_hops} hops" + (" (walk route)" if adj2 is None else "")
            if args.recommend_prefilter:
                show(route + " prefilter " + prefilter_name(args.recommend_prefilter),
                     rank_links(predictor, h, adj, adj2, first, truth, args.testbs, args, prefilter=args.recommend_prefilter,
                                hops=args.recommend_hops))
            show(route + (" unfiltered" if args.recommend_prefilter else ""),
                 rank_links(predictor, h, adj, adj2, first, truth, args.testbs, args, hops=args.recommend_hops))
    if args.recommend_explain:
        # --recommend-explain M: why these links — gradient x input on the pooled vectors, per common neighbour.  The winners form one
        # batch of their own: an unfrozen cn5 / cn7 weighs them by THAT batch's column statistics, so only a frozen predictor (or
        # cn8, which has no column weights) is explained at the scores the recommendation printed
        # (gradients want fp32 rows: main() refuses --table-dtype bf16 / f16 beside this option)
        h = table(adj)
        won = torch.stack([sources.view(-1, 1).expand_as(dst).reshape(-1), dst.reshape(-1)], dim=1)
        listed = won[:, 1] >= 0
        won = won[listed].contiguous()
        if won.shape[0]:
            exp = explain_links(predictor, h, adj, adj2, won, m=args.recommend_explain, args=args)
            frozen = predictor._frozen is not None
            diff = (exp.score - score.reshape(-1)[listed]).abs().max().item()
            print(f"explain: {won.shape[0]} links as one batch, predictor frozen = {frozen}; max |explained score - recommended "
                  f"score| = {diff:.2e}" + ("" if frozen else " (not frozen: the batch's own column weights, scores may differ)"),
                  flush=True)
            if frozen and not torch.allclose(exp.score, score.reshape(-1)[listed], rtol=1e-5, atol=1e-5):
                raise SystemExit("--recommend-explain: a frozen predictor's explained scores differ from the recommendation's")
            for (s, t), v, ks, cs, share in zip(won.tolist(), exp.score.tolist(), exp.nodes.tolist(), exp.contrib.tolist(),
                                                exp.pooled.tolist()):
                print(f"explain source {s} target {t} score {v:.4f} pooled {share[0]:+.4f} {share[1]:+.4f} top-{args.recommend_explain}: "
                      + " ".join(f"{n}({a:+.4f},{b:+.4f})" for n, (a, b) in zip(ks, cs) if n >= 0), flush=True)
    if args.recommend_explain_edges:
        # --recommend-explain-edges M: which links of the graph made the first printed recommendation look the way it does —
        # gradient x input on the messages of every conv layer (ocn_amd.explain.explain_link_edges), through the pooling and the
        # encoder.  The winners again form one batch; the explained candidate is its first row
        won = torch.stack([sources.view(-1, 1).expand_as(dst).reshape(-1), dst.reshape(-1)], dim=1)
        won = won[won[:, 1] >= 0].contiguous()
        if won.shape[0]:
            ex = explain_link_edges(model, predictor, data.x, adj, adj2, won, 0, top=args.recommend_explain_edges, args=args)
            s, t = won[0].tolist()
            print(f"explain-edges source {s} target {t} score {float(ex.score):.4f}: the {args.recommend_explain_edges} strongest messages "
                  f"of {ex.per_layer.shape[1]} conv layers, as col->row(total; per layer)", flush=True)
            for (r, c), v, per in zip(ex.entries.tolist(), ex.saliency.tolist(), ex.per_layer.tolist()):
                if r >= 0:
                    print(f"explain-edges message {c}->{r} ({v:+.3e}; " + " ".join(f"{p:+.3e}" for p in per) + ")", flush=True)
    if args.recommend_accept > 0:
        # --recommend-accept M: the M best of these links join the graph (ocn_amd.update.insert_edges: A and the stored A² are
        # updated, not rebuilt; the node embeddings are refreshed row by row, EncoderState) and the same sources are asked again
        pairs = torch.stack([sources.view(-1, 1).expand_as(dst).reshape(-1), dst.reshape(-1)])
        flat = score.reshape(-1).masked_fill(pairs[1] < 0, float("-inf"))
        best = flat.topk(min(args.recommend_accept, flat.numel())).indices
        accepted = pairs[:, best[pairs[1, best] >= 0]].contiguous()
        was, was2 = adj, adj2
        adj, adj2 = insert_edges(adj, accepted, adj2, donate=not args.recommend_undo)     # (an undo keeps the old pair to compare with)
        print(f"accepted {accepted.shape[1]} links: " + " ".join(f"{a}-{b}" for a, b in accepted.t().tolist()), flush=True)
        if state is not None:
            refreshed(adj, accepted, "accepting")
        dst, score = top(adj, adj2, "recommend after accepting")
        if args.recommend_undo:
            # --recommend-undo: the accepted links leave again (ocn_amd.update.remove_edges: A' = A \ D, the bits of A² that lose
            # their last witness cleared).  Recommended links are non-edges, so the round trip is exact
            adj, adj2 = remove_edges(adj, accepted, adj2, donate=True)
            if state is not None:
                refreshed(adj, accepted, "the undo")
            same = torch.equal(adj._rowptr, was._rowptr) and torch.equal(adj._col, was._col)
            if adj2 is not None:
                same = same and torch.equal(adj2._rowptr, was2._rowptr) and torch.equal(adj2._col, was2._col)
                if adj2.product_bit_rows() is not None and was2.product_bit_rows() is not None:
                    same = same and torch.equal(adj2.product_bit_rows(), was2.product_bit_rows())
            print(f"removed {accepted.shape[1]} links again: adj and adj2 restored exactly = {same}", flush=True)
            if not same:
                raise SystemExit("--recommend-undo: the restored graph differs from the original")
    return dst, score


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--dataset", default="cora")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--predictor", default="cn5", choices=sorted(predictor_dict))
    ap.add_argument("--model", default="puregcn")
    ap.add_argument("--hiddim", type=int, default=64)
    ap.add_argument("--mplayers", type=int, default=1)
    ap.add_argument("--nnlayers", type=int, default=3)
    ap.add_argument("--batch_size", type=int, default=1152)
    ap.add_argument("--testbs", type=int, default=8192)
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--maskinput", action="store_true")
    ap.add_argument("--adj2byblock", action="store_true")
    ap.add_argument("--use_valedges_as_input", action="store_true")
    ap.add_argument("--sum", type=float, default=0.0)
    ap.add_argument("--gnnlr", type=float, default=0.0043)
    ap.add_argument("--prelr", type=float, default=0.0024)
    ap.add_argument("--feat", type=int, default=0, help="feature width override for the synthetic x")
    ap.add_argument("--gnnedp", type=float, default=0.0, help="DropAdj probability of the encoder's adjacency (train only)")
    ap.add_argument("--res", action="store_true", help="residual connections in the encoder")
    # forwarded to the predictor for cn8 only, as the reference driver does (NeighborOverlap_large.py:210-214, 275-276)
    ap.add_argument("--beta", type=float, default=1)
    ap.add_argument("--use_xlin", action="store_true")
    ap.add_argument("--tailact", action="store_true")
    ap.add_argument("--twolayerlin", action="store_true")
    ap.add_argument("--heuristic", default=None, choices=KINDS, help="skip training: print the dataset's metric for this link heuristic")
    ap.add_argument("--recommend", type=int, default=0, metavar="K",
                    help="after the last epoch (at once with --heuristic): print the top-K predicted targets of the first few test sources")
    ap.add_argument("--structured-negatives", action="store_true",
                    help="draw the training negatives (and citation2's evaluation negatives) from the non-edges on the device "
                         "(ocn_amd.sampling) instead of torch.randint pairs, which can be links")
    ap.add_argument("--hard-negatives", type=float, default=0.0, metavar="SHARE",
                    help="share in [0, 1] of the training positives whose negative is the 2-hop corruption of their target "
                         "(ocn_amd.sampling.two_hop_negative_edges): positive t when t %% 100 < round(100 * SHARE); the others keep "
                         "the draw of --structured-negatives / torch.randint.  0: that draw alone")
    ap.add_argument("--hard-eval-negatives", action="store_true",
                    help="citation2's evaluation negatives from the 2-hop candidates of each source "
                         "(ocn_amd.sampling.two_hop_negative_targets) where --structured-negatives draws uniform non-links")
    ap.add_argument("--recommend-walk", action="store_true",
                    help="--recommend without A² (adj2=None): for graphs whose A² cannot be formed; 1-hop heuristics or the model")
    ap.add_argument("--recommend-frozen", action="store_true",
                    help="with --recommend and a cn5 / cn7 model: freeze the column weights on the validation positives "
                         "(ocn_amd.frozen) so that a source's scores do not depend on the other sources or the batch size")
    ap.add_argument("--recommend-hops", type=int, default=2, choices=(2, 3),
                    help="with --recommend: candidates within this many hops (recommend_links(hops=...)); 3 reaches the pairs whose "
                         "only evidence is cn2, and takes --recommend-prefilter KIND:M:DECAY")
    ap.add_argument("--recommend-prefilter", default=None, metavar="KIND:M[:DECAY]",
                    help="with --recommend and a model: short-list the M best candidates per source by the heuristic KIND (cn, aa or "
                         "ra; K <= M <= 128) and let the model rank only those (recommend_links(prefilter=...))")
    ap.add_argument("--recommend-long", default=None, metavar="KIND:M[:DECAY]",
                    help="with --recommend and a model, instead of --recommend-prefilter: the same short list for any M >= K "
                         "(ocn_amd.recommend.PathSums: the M best as a set through ocn_segment_keep_best; no limit of 128)")
    ap.add_argument("--recommend-rw", default=None, metavar="M:W:L[:DECAY]",
                    help="with --recommend and a model, instead of --recommend-prefilter: short-list the M most visited nodes of W "
                         "random walks of L = --recommend-hops steps per source (ocn_amd.recommend.RandomWalks; DECAY with L = 3) and "
                         "let the model rank only those; with --recommend-eval, coverage reads 'visited at all'")
    ap.add_argument("--recommend-emb", default=None, metavar="M[:cos]",
                    help="with --recommend and a model: short-list the M nodes nearest to the source's embedding by exact int8 inner "
                         "product over ALL nodes (ocn_amd.recommend.EmbeddingNeighbours; ':cos' normalises the rows first) and let the "
                         "model rank only those; alone, or with --recommend-union beside another short list")
    ap.add_argument("--recommend-union", action="store_true",
                    help="with --recommend-emb and one of --recommend-prefilter / --recommend-rw: the model ranks the per-source union "
                         "of the two short lists (ocn_amd.recommend.ShortListUnion); with --recommend-eval, coverage reads 'in the union'")
    ap.add_argument("--recommend-eval", type=int, default=0, metavar="Q",
                    help="with --recommend: rank the held-out test links of the first Q distinct test sources among the candidates of "
                         "the selected route (ocn_amd.ranking) and print recall / NDCG / hit rate @K, MRR, coverage and, with "
                         "--recommend-prefilter, retention beside the unfiltered run")
    ap.add_argument("--recommend-explain", type=int, default=0, metavar="M",
                    help="with --recommend and a cn5 / cn7 / cn8 model: explain the K winners of the printed sources as one batch "
                         "(ocn_amd.explain) and print each target's top-M common neighbours with their two contributions")
    ap.add_argument("--recommend-explain-edges", type=int, default=0, metavar="M",
                    help="with --recommend and a cn5 / cn7 / cn8 model: list the M strongest messages (links of the graph, per conv "
                         "layer) behind the first printed recommendation (ocn_amd.explain.explain_link_edges)")
    ap.add_argument("--recommend-accept", type=int, default=0, metavar="M",
                    help="with --recommend: insert the M best recommended links into the graph (ocn_amd.update) and recommend again")
    ap.add_argument("--recommend-undo", action="store_true",
                    help="with --recommend-accept: remove the accepted links again (ocn_amd.update.remove_edges) and check that the "
                         "adjacency and A² are restored exactly")
    ap.add_argument("--recommend-check-refresh", action="store_true",
                    help="with --recommend-accept and a model: assert that the refreshed node embeddings (ocn_amd.update.EncoderState) "
                         "equal a full encoder pass bit for bit after the insert, and after the undo")
    ap.add_argument("--table-dtype", choices=("fp32", "bf16", "f16", "int8"), default="fp32",
                    help="the embedding table the predictor pools from in test() and under --recommend (pipeline.embedding_table): "
                         "bf16 / f16 rows are half the bytes, widened exactly and summed in fp32; int8 rows with a scale per row are "
                         "a quarter, the image --recommend-emb retrieves from, and may be capped (--cn-cap); training is always fp32")
    ap.add_argument("--cn-cap", default=None, metavar="D[:SEED]",
                    help="test() and --recommend pool at most D embedding rows per candidate (predictor.set_cn_cap): a stratified, "
                         "reweighted sample of its common neighbours, fixed by SEED (default 0); training always pools exactly")
    args = ap.parse_args(argv)
    if args.cn_cap is not None:
        parts = args.cn_cap.split(":")
        if not (1 <= len(parts) <= 2 and all(p.isdigit() for p in parts) and int(parts[0]) >= 1):
            ap.error("--cn-cap D[:SEED]: D >= 1 rows per candidate, SEED a non-negative integer")
        if (args.heuristic or args.predictor == "cn6" or args.table_dtype not in ("fp32", "int8") or args.recommend_explain
                or args.recommend_explain_edges):
            ap.error("--cn-cap: needs a cn5, cn7 or cn8 model and an fp32 or int8 table; the explanations explain the exact pooling")
        args.cn_cap = (int(parts[0]), int(parts[1]) if len(parts) == 2 else 0)
    if args.table_dtype != "fp32" and (args.predictor == "cn6" or args.recommend_explain or args.recommend_explain_edges
                                       or (args.recommend_emb and (args.table_dtype != "int8" or args.recommend_emb.endswith(":cos")))):
        ap.error("--table-dtype bf16 / f16 / int8: cn6, --recommend-explain, --recommend-explain-edges and --recommend-emb read fp32 "
                 "rows (int8: --recommend-emb M retrieves from the table itself, M:cos needs the fp32 rows)")
    if not 0.0 <= args.hard_negatives <= 1.0:
        ap.error("--hard-negatives SHARE: a share in [0, 1]")
    if args.recommend_check_refresh and (args.heuristic or not (args.recommend and args.recommend_accept > 0)):
        ap.error("--recommend-check-refresh: needs a model and --recommend K --recommend-accept M")
    if args.recommend_undo and not (args.recommend and args.recommend_accept > 0):
        ap.error("--recommend-undo: needs --recommend K --recommend-accept M")
    if args.recommend_walk and args.heuristic in TWO_HOP:
        ap.error("--recommend-walk: a 2-hop heuristic intersects with the rows of A²")
    if args.recommend_frozen and (args.heuristic or not args.recommend or args.predictor not in ("cn5", "cn7")):
        ap.error("--recommend-frozen: needs --recommend K and a cn5 or cn7 model")
    if args.recommend_explain and (args.heuristic or not args.recommend or args.predictor == "cn6"
                                   or not 1 <= args.recommend_explain <= 128):
        ap.error("--recommend-explain M: needs --recommend K, a cn5, cn7 or cn8 model and 1 <= M <= 128")
    if args.recommend_explain_edges and (args.heuristic or not args.recommend or args.predictor == "cn6"
                                         or not 1 <= args.recommend_explain_edges <= 128):
        ap.error("--recommend-explain-edges M: needs --recommend K, a cn5, cn7 or cn8 model and 1 <= M <= 128")
    if args.recommend_hops != 2 and not args.recommend:
        ap.error("--recommend-hops: needs --recommend K")
    if args.recommend_eval < 0 or (args.recommend_eval and not args.recommend):
        ap.error("--recommend-eval Q: needs --recommend K and Q >= 1")
    if args.recommend_prefilter:
        parts = args.recommend_prefilter.split(":")
        kind, m, decay = parts[0], "".join(parts[1:2]), parts[2:]
        if args.heuristic or not args.recommend or kind not in ("cn", "aa", "ra") or not m.isdigit() or not args.recommend <= int(m) <= 128:
            ap.error("--recommend-prefilter KIND:M: needs a model, --recommend K, KIND one of cn, aa, ra and K <= M <= 128")
        if len(decay) != args.recommend_hops - 2:
            ap.error("--recommend-prefilter: KIND:M with --recommend-hops 2, KIND:M:DECAY with --recommend-hops 3")
        args.recommend_prefilter = (kind, int(m))
        if decay:
            try:
                d = float(decay[0])
            except ValueError:
                d = -1.0
            if not (math.isfinite(d) and d >= 0):
                ap.error("--recommend-prefilter KIND:M:DECAY: DECAY is a finite number >= 0")
            args.recommend_prefilter += (d,)
    if args.recommend_long:
        if args.recommend_prefilter:
            ap.error("--recommend-long and --recommend-prefilter are two short lists: give one")
        if args.heuristic or not args.recommend:
            ap.error("--recommend-long KIND:M[:DECAY]: needs a model and --recommend K")
        parts = args.recommend_long.split(":")
        try:
            if len(parts) != args.recommend_hops:
                raise ValueError("KIND:M with --recommend-hops 2, KIND:M:DECAY with --recommend-hops 3")
            stage = PathSums(parts[0], int(parts[1]), float(parts[2]) if len(parts) == 3 else None)
            if args.recommend > stage.m:
                raise ValueError(f"M = {stage.m} is fewer than K = {args.recommend}")
        except ValueError as e:
            ap.error(f"--recommend-long KIND:M[:DECAY]: {e}")
        args.recommend_prefilter = stage         # (one short list per request: the calls below pass it as prefilter=)
    if args.recommend_rw:
        if args.recommend_prefilter:
            ap.error("--recommend-rw and --recommend-prefilter / --recommend-long are two short lists: give one")
        if args.heuristic or not args.recommend:
            ap.error("--recommend-rw M:W:L[:DECAY]: needs a model and --recommend K")
        parts = args.recommend_rw.split(":")
        try:
            if not 3 <= len(parts) <= 4:
                raise ValueError("M:W:L with --recommend-hops 2, M:W:L:DECAY with --recommend-hops 3")
            rw = RandomWalks(int(parts[0]), int(parts[1]), int(parts[2]), float(parts[3]) if len(parts) == 4 else None)
            if rw.length != args.recommend_hops:
                raise ValueError(f"L = {rw.length} steps, --recommend-hops {args.recommend_hops}: the two must be equal")
            if args.recommend > rw.m:
                raise ValueError(f"M = {rw.m} is fewer than K = {args.recommend}")
        except ValueError as e:
            ap.error(f"--recommend-rw M:W:L[:DECAY]: {e}")
        args.recommend_prefilter = rw            # (one short list per request: the calls below pass it as prefilter=)
    if args.recommend_union and not (args.recommend_emb and args.recommend_prefilter):
        ap.error("--recommend-union: needs --recommend-emb and one of --recommend-prefilter / --recommend-rw")
    if args.recommend_emb:
        if args.heuristic or not args.recommend:
            ap.error("--recommend-emb M[:cos]: needs a model and --recommend K")
        if args.recommend_prefilter and not args.recommend_union:
            ap.error("--recommend-emb beside another short list: give --recommend-union to rank their union")
        parts = args.recommend_emb.split(":")
        try:
            if not 1 <= len(parts) <= 2 or (len(parts) == 2 and parts[1] != "cos"):
                raise ValueError("M, or M:cos")
            emb = EmbeddingNeighbours(int(parts[0]), normalize=len(parts) == 2)
            if args.recommend > max(emb.m, 0 if not args.recommend_union else
                                    (args.recommend_prefilter.m if isinstance(args.recommend_prefilter, (RandomWalks, PathSums)) else args.recommend_prefilter[1])):
                raise ValueError(f"M = {emb.m} is fewer than K = {args.recommend}")
        except ValueError as e:
            ap.error(f"--recommend-emb M[:cos]: {e}")
        args.recommend_prefilter = ShortListUnion(args.recommend_prefilter, emb) if args.recommend_union else emb
    dev = torch.device("cuda:0")
    evaluator = Evaluator(name='ogbl-ppa' if args.dataset in ("cora", "citeseer", "pubmed") else f'ogbl-{args.dataset}')
    data, split_edge = loaddataset_like(args.dataset, args.use_valedges_as_input, scale=args.scale, feat=args.feat)
    data.x = data.x.to(dev)
    data.adj_t = data.adj_t.to_device(dev)
    data.full_adj_t = data.full_adj_t.to_device(dev) if args.use_valedges_as_input else data.adj_t
    if args.heuristic:
        if evaluator.eval_metric == "mrr":
            ap.error("--heuristic: this driver scores the Hits@K datasets (as its test() does)")
        res = test_heuristic(args.heuristic, data, split_edge, evaluator, args.testbs, args)
        print(f"heuristic {args.heuristic} {evaluator.eval_metric} valid/test {res['valid']:.4f}/{res['test']:.4f}", flush=True)
        if args.recommend:
            recommend(args.recommend, data, split_edge, args)
        return res
    torch.manual_seed(0)
    fin = args.hiddim if data.max_x >= 0 else data.x.shape[1]
    model = GCN(fin, args.hiddim, args.hiddim, args.mplayers, 0.05, True, args.res, data.max_x, args.model, True, args.gnnedp,
                xdropout=0.3, taildropout=0.1).to(dev)
    heads = (dict(use_xlin=args.use_xlin, tailact=args.tailact, twolayerlin=args.twolayerlin, beta=args.beta)
             if args.predictor == "cn8" else dict(use_xlin=True, tailact=True))
    predictor = predictor_dict[args.predictor](args.hiddim, args.hiddim, 1, args.nnlayers, 0.05, 0.0, True, **heads).to(dev)
    optimizer = torch.optim.Adam([{'params': model.parameters(), "lr": args.gnnlr},
                                  {'params': predictor.parameters(), 'lr': args.prelr}])
    out = []
    for epoch in range(1, 1 + args.epochs):
        t1 = time.time()
        loss = train(model, predictor, data, split_edge, optimizer, args.batch_size, args.maskinput, args, epoch)
        t2 = time.time()
        run_test = test_mrr if evaluator.eval_metric == "mrr" else test
        if args.cn_cap is not None:                      # --cn-cap: the evaluation pools a capped sample, the next epoch trains exactly
            predictor.set_cn_cap(*args.cn_cap)
        results, _ = run_test(model, predictor, data, split_edge, evaluator, args.testbs, args.use_valedges_as_input, args)
        predictor.set_cn_cap(None)
        torch.cuda.synchronize()
        t3 = time.time()
        line = (f"epoch {epoch:3d} loss {loss:.4f} train {t2 - t1:.2f}s test {t3 - t2:.2f}s  " +
                "  ".join(f"{k} {'train/valid/test' if len(v) == 3 else 'valid/test'} " + "/".join(f"{x:.3f}" for x in v)
                          for k, v in results.items()))
        print(line, flush=True)
        out.append((loss, results))
    if args.recommend:
        if args.cn_cap is not None:
            predictor.set_cn_cap(*args.cn_cap)
        recommend(args.recommend, data, split_edge, args, model, predictor)
    return out


if __name__ == "__main__":
    main()
