"""Batched multi-sentence beam search.

Serving-throughput extension beyond the reference (which decodes one
sentence per process, gen.py:30-45): S sentences' beams share every
decode step as one (S*k)-row batch through the fused decoder kernels
(row budget: the cond-GRU kernels take B <= 32). Per-sentence semantics
are identical to decode.beam.gen_sample — sources are padded to the
longest and masked via ctx_mask, so attention, the distraction terms and
the histories are unaffected by padding.

Execution layout (MI355X): all recurrent state (h2, acc_ctx, acc_alpha,
rerank histories) stays device-resident across steps and hypothesis
reshuffles are device index_selects; the only per-step host transfers
are the top-k candidate ids/costs and the selected attention rows for
the alignment output (two small synchronisations per step — the naive
numpy bookkeeping round-trip was ~25% of decode time in the kernel
trace, profiles/decode_kernel_stats.csv). With ``fused_select=True`` the
per-sentence top-k loop becomes one ops.beam_select call per step
(measured in profiles/README.md, "Decode v4"). With ``paged_rerank=True``
the rerank histories of all sentences live in one ops.RerankHistory: each
step's rows are stored once and an int32 ancestor table is reshuffled
instead of the histories themselves (docs/DESIGN.md, "Rerank histories").
With ``shared_ctx=True`` the per-sentence context is never expanded to one
column per hypothesis row: it is rounded to bf16 once per micro-batch and
the attention kernel reads it through the row -> sentence table
(ops.cond_gru_step_shared; profiles/README.md, "Decode v6").
With ``resident_state=True`` the hypothesis rows stay in the stepper's input
buffers: the host keeps deciding, uploads one table of next-step rows per
step, and one ops.beam_reorder launch replaces the per-sentence
index_selects, uploads and concatenations; the alignments' attention rows
are logged on the device and fetched once (docs/DESIGN.md, "Resident beam
rows"; profiles/README.md, "Decode v7").

Numerics note: results are mathematically identical to per-sentence
gen_sample, but not bitwise — the batched masked-mean init state and
torch reductions over different padded lengths round differently at the
last ulp. On a trained model beams are insensitive to this; a
random-init model with near-tie hypotheses can flip a beam choice
(observed only with inflated-readout test models).
"""

import math

import numpy
import torch

from .. import ops
from .beam import distraction_penalties_gpu


def _select_fused(st, dstate, alive, k, ii, probs, alpha, ctx_t, h2, use_unk,
                  any_lambda, kl_factor, ctx_factor, state_factor,
                  paged_pen=None, gather_alpha=True):
    """Phases 1 and 2a of a decode step through ops.beam_select: one upload
    ([running scores | seg_off | want], the fp32 scores carried as their
    int32 bits), one selection call for every alive sentence, one copy of
    the ranks/costs back, one gather of every selected attention row.

    Returns (pend, alpha_sel) exactly as the per-sentence path builds
    them: pend[j] = (i, sl, tis, wis, costs, sel_dev) per alive sentence,
    alpha_sel the selected attention rows in pend order (host array).
    ``paged_pen``: the (R,) rerank penalties of a RerankHistory, used in
    place of the per-sentence ones. ``gather_alpha=False`` (resident_state:
    the alignments come from the device log at the end) skips the attention
    gather and its copy; alpha_sel is then None."""
    device = probs.device
    V = probs.shape[1]
    lives = [st[i]["live"] for i in alive]
    wants = [k - st[i]["dead"] for i in alive]
    Sa, R, K = len(alive), sum(lives), max(wants)
    seg = numpy.zeros(Sa + 1, dtype="int32")
    seg[1:] = numpy.cumsum(lives)
    prev = numpy.concatenate([st[i]["scores"] for i in alive])
    tab = torch.from_numpy(numpy.concatenate(
        [prev.astype("float32").view("int32"), seg,
         numpy.asarray(wants, dtype="int32")])).to(device)
    prev_dev = tab[:R].view(torch.float32)
    seg_dev, want_dev = tab[R:R + Sa + 1], tab[R + Sa + 1:]

    # rerank penalties stay per sentence (zeros where there is no history)
    penalty = None
    if ii > 0 and paged_pen is not None:
        penalty = paged_pen
    elif ii > 0 and any_lambda:
        pens = []
        for j, i in enumerate(alive):
            sl = slice(int(seg[j]), int(seg[j + 1]))
            if dstate[i]["ha"] is None:
                pens.append(torch.zeros(lives[j], device=device))
                continue
            pens.append(distraction_penalties_gpu(
                dstate[i]["ha"], dstate[i]["hc"], dstate[i]["hs"],
                alpha[sl].float(), ctx_t[sl].float(), h2[sl].float(),
                kl_factor, ctx_factor, state_factor))
        penalty = torch.cat(pens)

    ranks_dev, costs_dev = ops.beam_select(
        probs.float(), prev_dev, seg_dev, want_dev, penalty=penalty,
        use_unk=use_unk, K=K)
    # batch row of every selection (padding slots point at row seg[s]):
    # for the attention gather and the dense rerank histories
    need_rows = gather_alpha or (any_lambda and paged_pen is None)
    if need_rows:
        rows_dev = ranks_dev.clamp_min(0) // V + seg_dev[:-1, None]
    sel_host = torch.cat([ranks_dev.double().flatten(),
                          costs_dev.double().flatten()]).cpu().numpy()
    if gather_alpha:
        alpha_pad = alpha.float()[rows_dev.flatten()].cpu().numpy()

    pend, alpha_rows = [], []
    for j, i in enumerate(alive):
        sl = slice(int(seg[j]), int(seg[j + 1]))
        want = wants[j]
        ranks = sel_host[j * K:j * K + want].astype(numpy.int64)
        costs = sel_host[(Sa + j) * K:(Sa + j) * K + want].astype("float32")
        pend.append((i, sl, ranks // V, ranks % V, costs,
                     rows_dev[j, :want] if need_rows else None))
        if gather_alpha:
            alpha_rows.append(alpha_pad[j * K:j * K + want])
    return pend, numpy.concatenate(alpha_rows) if gather_alpha else None


@torch.no_grad()
def gen_sample_batched(model, xs, k=1, maxlen=30, use_unk=False,
                       kl_factor=0.0, ctx_factor=0.0, state_factor=0.0,
                       use_graph=True, fused_select=False,
                       paged_rerank=False, shared_ctx=False,
                       resident_state=False):
    """Beam-decode a list of sources jointly.

    fused_select: pick every sentence's candidates with one
    ops.beam_select call per step (one table upload, one result copy)
    instead of the per-sentence topk loop. Same keys; exactly equal keys
    go to the lower flat index (topk leaves that choice open). Opt-in.

    paged_rerank: keep the distraction-rerank histories of all sentences
    in one ops.RerankHistory (slabs written once per step + an ancestor
    table) and compute every row's penalties in one call per step, instead
    of re-gathering dense per-sentence histories. Same penalties bit for
    bit; a no-op when all three factors are 0. Opt-in.

    shared_ctx: attend every hypothesis row to its sentence's column of
    the per-sentence context (bf16, rounded once) through the sent_idx
    table, instead of gathering ctx / pctx / mask to one column per row
    and re-rounding them on every step. Same results bit for bit. Opt-in.

    resident_state: the hypothesis rows stay in the stepper's input
    buffers. The host decides as ever (samples, scores, dead counts, EOS);
    per step it uploads one (3, L) table [parent row | word | sentence] of
    the next step's rows and one ops.beam_reorder call moves h2 / acc_ctx /
    acc_alpha from the step's outputs into its inputs, writes the words and
    the routing and pads the tail, in place of the per-sentence
    index_selects, uploads and concatenations. Attention rows are logged
    on the device per step and fetched once at the end for the alignments.
    Every value is a copy of what the default path produces: same results
    bit for bit. Opt-in.

    xs: list of (T_i, 1) int64 tensors (same device as model).
    maxlen: an int, or a per-sentence list (serving: each request brings
    its own cap — a sentence whose cap is reached flushes its live
    hypotheses and drops out of the shared batch, gen_sample
    semantics nats.py:1068-1074 per sentence).
    Returns a list of (sample, sample_score, sample_dec_alphas) tuples,
    one per sentence, each shaped exactly like gen_sample's beam output
    (alignment alphas are trimmed to the sentence's own length).
    """
    S = len(xs)
    assert S >= 1
    maxlens = ([int(maxlen)] * S if isinstance(maxlen, int)
               else [int(m) for m in maxlen])
    assert len(maxlens) == S
    device = xs[0].device
    any_lambda = (kl_factor > 0.0 or ctx_factor > 0.0 or state_factor > 0.0)
    paged = bool(paged_rerank) and any_lambda
    history = None  # ops.RerankHistory, built at the first step

    # ONE batched masked encode for all sentences (identical per-column to
    # each sentence's own unpadded encode — see f_init): pads to the
    # longest source so the encoder scans run S columns per launch instead
    # of S separate T-step launches.
    lens = [int(x.shape[0]) for x in xs]
    Ts = max(lens)
    if use_graph and device.type == "cuda":
        # bucket the padded source length so serving traffic with varied
        # lengths reuses a handful of captured graphs instead of one per
        # distinct Ts (padding is exact: ctx_mask zeroes the pad columns
        # through attention and the encoder mask-blend)
        Ts = (Ts + 63) // 64 * 64
    x_pad = torch.zeros(Ts, S, dtype=torch.int64, device=device)
    src_mask = torch.zeros(Ts, S, device=device)
    for i, x in enumerate(xs):
        x_pad[:lens[i], i] = x[:, 0]
        src_mask[:lens[i], i] = 1.0
    init_all, ctx_all = model.f_init(x_pad, src_mask)
    C = ctx_all.shape[2]

    # per-sentence host bookkeeping (sample token lists + scores; identical
    # math to gen_sample) — everything tensor-valued lives on device
    # prows (paged rerank): the batch row of this step that each live
    # hypothesis continues, as host ints
    st = [dict(live=1, dead=0, samples=[[]], prows=[],
               scores=numpy.zeros(1, dtype="float32"),
               alphas=[[]], out_samples=[], out_scores=[], out_alphas=[])
          for _ in range(S)]
    dstate = [dict(state=init_all[i:i + 1],
                   w=torch.full((1,), -1, dtype=torch.int64, device=device),
                   acc_c=torch.zeros(1, C, device=device),
                   acc_a=torch.zeros(1, Ts, device=device),
                   ha=None, hc=None, hs=None)
              for i in range(S)]

    ctx_pad = torch.zeros(Ts, S, C, device=device, dtype=ctx_all.dtype)
    for i in range(S):
        ctx_pad[:lens[i], i] = ctx_all[:lens[i], i]
    ctx_mask_s = src_mask
    graphed = use_graph and device.type == "cuda"
    if shared_ctx and not graphed:
        # bf16 once per micro-batch; pctx from the fp32 context as ever
        ctx_dec, cmask_dec, pctx_pad = model.decode_context(ctx_pad,
                                                            ctx_mask_s)
    else:
        pctx_pad = model.project_ctx(ctx_pad)

    # hipGraph-captured f_next for the shared step (fixed row budget S*k;
    # the per-step sentence gather, or with shared_ctx the row -> sentence
    # table read, runs inside the graph)
    stepper = None
    if graphed:
        from .graph import get_batched_stepper
        stepper = get_batched_stepper(model, ctx_pad.float(), ctx_mask_s,
                                      pctx_pad.float(), S * k,
                                      shared_ctx=shared_ctx)
    resident = bool(resident_state)
    if resident and stepper is None:
        # the same buffers without a graph: one code path below for both
        from .graph import RowStepper
        if shared_ctx:
            stepper = RowStepper(model, ctx_dec, cmask_dec, pctx_pad, S * k,
                                 shared_ctx=True)
        else:
            stepper = RowStepper(model, ctx_pad, ctx_mask_s, pctx_pad, S * k)
    table_dev = None  # resident: the (3, L) table of the step to run
    alog = None       # resident: (max(maxlens), S*k, Ts) log of alpha rows

    NEG_UNK = math.log(1e-20)

    for ii in range(max(maxlens)):
        # sentences at their own maxlen flush live hypotheses and leave
        for i in range(S):
            if st[i]["live"] > 0 and ii >= maxlens[i]:
                for idx2 in range(st[i]["live"]):
                    st[i]["out_samples"].append(st[i]["samples"][idx2])
                    st[i]["out_scores"].append(float(st[i]["scores"][idx2]))
                    st[i]["out_alphas"].append(st[i]["alphas"][idx2])
                st[i].update(samples=[], alphas=[],
                             scores=numpy.zeros(0, dtype="float32"))
                st[i]["live"] = 0
        alive = [i for i in range(S) if st[i]["live"] > 0]
        if not alive:
            break
        if resident and ii > 0:
            # the rows are in the stepper's buffers already (beam_reorder
            # at the end of the previous step)
            rows = table_dev.shape[1]
            parent_dev = table_dev[0]
            probs, h2, alpha, ctx_t, acc_c, acc_a = [
                o[:rows] for o in stepper.replay(rows)]
        else:
            sent_rows = sum(([i] * st[i]["live"] for i in alive), [])
            if paged:
                # the parents of the ancestor-table advance ride along with
                # sent_idx: one upload for both
                up = torch.tensor(
                    sent_rows + sum((st[i]["prows"] for i in alive), []),
                    device=device)
                sent_idx, parent_dev = up[:len(sent_rows)], up[len(sent_rows):]
            elif stepper is not None or not shared_ctx:
                sent_idx = torch.tensor(sent_rows, device=device)
            y = torch.cat([dstate[i]["w"] for i in alive])
            state = torch.cat([dstate[i]["state"] for i in alive])
            acc_c = torch.cat([dstate[i]["acc_c"] for i in alive])
            acc_a = torch.cat([dstate[i]["acc_a"] for i in alive])
            if stepper is None and not shared_ctx:
                ctx_b = ctx_pad[:, sent_idx]
                cmask_b = ctx_mask_s[:, sent_idx]
                pctx_b = pctx_pad[:, sent_idx]

            if stepper is not None:
                rows = y.shape[0]
                outs = stepper.step(sent_idx, y, state.float(), acc_c.float(),
                                    acc_a.float())
                probs, h2, alpha, ctx_t, acc_c, acc_a = [
                    o[:rows] for o in outs]
            elif shared_ctx:
                probs, _, h2, alpha, ctx_t, acc_c, acc_a = model.f_next(
                    y, ctx_dec, cmask_dec, pctx_pad, state, acc_c, acc_a,
                    sample_draw=False,
                    row_src=sent_rows)  # validated, 1 upload
            else:
                probs, _, h2, alpha, ctx_t, acc_c, acc_a = model.f_next(
                    y, ctx_b, cmask_b, pctx_b, state, acc_c, acc_a,
                    sample_draw=False)
        V = probs.shape[1]

        paged_pen = None
        if paged:
            if history is None:
                history = ops.RerankHistory(
                    max(maxlens), S * k, alpha.shape[1], ctx_t.shape[1],
                    h2.shape[1], device)
            paged_pen = history.step(
                parent_dev, alpha.float().contiguous(),
                ctx_t.float().contiguous(), h2.float().contiguous(),
                (kl_factor, ctx_factor, state_factor))

        if resident:
            # every row's attention, before selection: the alignments are
            # gathered from this log once, after the last step
            if paged:
                alog = history.hist_a  # the rerank slab already is that log
            else:
                if alog is None:
                    alog = torch.empty(max(maxlens), S * k, alpha.shape[1],
                                       device=device)
                alog[ii, :rows] = alpha
        # the selected rows as a device tensor: only the dense rerank
        # histories still need them when the rows stay resident
        need_sel = not resident or (any_lambda and not paged)

        if fused_select:
            pend, alpha_sel = _select_fused(
                st, dstate, alive, k, ii, probs, alpha, ctx_t, h2, use_unk,
                any_lambda, kl_factor, ctx_factor, state_factor, paged_pen,
                gather_alpha=not resident)
        else:
            # -- phase 1: per-sentence top-k ON DEVICE, one host transfer --
            logp = probs.float().log()
            if not use_unk:
                logp[:, 1] = NEG_UNK
            # per alive sentence: (ranks (want,), costs (want,))
            sel_parts = []
            row0 = 0
            for i in alive:
                live = st[i]["live"]
                sl = slice(row0, row0 + live)
                row0 += live
                cand = torch.as_tensor(st[i]["scores"],
                                       device=device)[:, None] - logp[sl]
                cand_flat = cand.flatten()
                want = k - st[i]["dead"]
                sel_flat = cand_flat
                if ii > 0 and paged:
                    sel_flat = (cand + paged_pen[sl, None]).flatten()
                elif ii > 0 and any_lambda and dstate[i]["ha"] is not None:
                    pen = distraction_penalties_gpu(
                        dstate[i]["ha"], dstate[i]["hc"], dstate[i]["hs"],
                        alpha[sl].float(), ctx_t[sl].float(), h2[sl].float(),
                        kl_factor, ctx_factor, state_factor)
                    sel_flat = (cand + pen[:, None]).flatten()
                ranks = sel_flat.topk(want, largest=False).indices
                # UN-reranked costs
                sel_parts.append((ranks, cand_flat[ranks]))
            flat_host = torch.cat([torch.cat([r.double(), c.double()])
                                   for r, c in sel_parts]).cpu().numpy()

            # -- phase 2: bookkeeping + device-side state reshuffle --
            alpha_gather = []   # device rows to fetch for alignments
            pend = []           # (i, sl, tis, wis, costs, sel_dev)
            row0 = 0
            off = 0
            for i in alive:
                live = st[i]["live"]
                sl = slice(row0, row0 + live)
                row0 += live
                want = k - st[i]["dead"]
                ranks = flat_host[off:off + want].astype(numpy.int64)
                costs = flat_host[off + want:off + 2 * want].astype("float32")
                off += 2 * want
                tis = ranks // V
                wis = ranks % V
                sel_dev = None
                if need_sel:
                    sel_dev = torch.as_tensor(tis, device=device) + sl.start
                if not resident:
                    alpha_gather.append(alpha.float()[sel_dev])
                pend.append((i, sl, tis, wis, costs, sel_dev))
            alpha_sel = None
            if not resident:
                alpha_sel = torch.cat(alpha_gather).cpu().numpy()

        arow = 0
        tab_p, tab_w, tab_s = [], [], []  # resident: the next step's rows
        for i, sl, tis, wis, costs, sel_dev in pend:
            want = len(tis)
            if not resident:
                a_np = alpha_sel[arow:arow + want]
            arow += want

            new_samples, new_scores, new_alphas, new_words = [], [], [], []
            for r, (ti, wi) in enumerate(zip(tis, wis)):
                new_samples.append(st[i]["samples"][ti] + [int(wi)])
                new_scores.append(float(costs[r]))
                # resident: (step, batch row) into the device log
                new_alphas.append(st[i]["alphas"][ti] + [
                    (ii, sl.start + int(ti)) if resident
                    else a_np[r, :lens[i]].copy()])
                new_words.append(int(wi))

            # device histories for the rerank (pre-filter selection order)
            if any_lambda and not paged:
                cur_a = alpha.float()[sel_dev].unsqueeze(0)
                cur_c = ctx_t.float()[sel_dev].unsqueeze(0)
                cur_s = h2.float()[sel_dev].unsqueeze(0)
                if dstate[i]["ha"] is None:
                    ha, hc, hs = cur_a, cur_c, cur_s
                else:
                    ti_dev = sel_dev - sl.start
                    ha = torch.cat([dstate[i]["ha"][:, ti_dev], cur_a], 0)
                    hc = torch.cat([dstate[i]["hc"][:, ti_dev], cur_c], 0)
                    hs = torch.cat([dstate[i]["hs"][:, ti_dev], cur_s], 0)

            keep, samples, scores, alphas_l, words_l = [], [], [], [], []
            for idx2 in range(want):
                if new_samples[idx2][-1] == 0:
                    st[i]["out_samples"].append(new_samples[idx2])
                    st[i]["out_scores"].append(new_scores[idx2])
                    st[i]["out_alphas"].append(new_alphas[idx2])
                    st[i]["dead"] += 1
                else:
                    keep.append(idx2)
                    samples.append(new_samples[idx2])
                    scores.append(new_scores[idx2])
                    alphas_l.append(new_alphas[idx2])
                    words_l.append(new_words[idx2])

            st[i].update(samples=samples, alphas=alphas_l,
                         scores=numpy.array(scores, dtype="float32"))
            st[i]["live"] = len(samples)
            if st[i]["dead"] >= k:
                st[i]["live"] = 0
            if st[i]["live"] > 0 and resident:
                # a sentence at its cap after this step leaves the table
                if ii + 1 < maxlens[i]:
                    tab_p += [sl.start + int(tis[j]) for j in keep]
                    tab_w += words_l
                    tab_s += [i] * len(keep)
                if any_lambda and not paged:
                    kt = torch.tensor(keep, dtype=torch.int64, device=device)
                    dstate[i]["ha"] = ha[:, kt]
                    dstate[i]["hc"] = hc[:, kt]
                    dstate[i]["hs"] = hs[:, kt]
            elif st[i]["live"] > 0:
                kt = torch.tensor(keep, dtype=torch.int64, device=device)
                sel_keep = sel_dev[kt]
                dstate[i]["w"] = torch.tensor(words_l, dtype=torch.int64,
                                              device=device)
                dstate[i]["state"] = h2[sel_keep].float()
                dstate[i]["acc_c"] = acc_c[sel_keep].float()
                dstate[i]["acc_a"] = acc_a[sel_keep].float()
                if paged:
                    st[i]["prows"] = [sl.start + int(tis[j]) for j in keep]
                elif any_lambda:
                    dstate[i]["ha"] = ha[:, kt]
                    dstate[i]["hc"] = hc[:, kt]
                    dstate[i]["hs"] = hs[:, kt]

        if tab_p:
            # one upload, one launch: the kept rows move from this step's
            # outputs into the next step's inputs, with their words, their
            # routing and the padding tail
            dsts, y_buf, route_buf = stepper.resident_buffers()
            table_dev = ops.beam_reorder(
                [tab_p, tab_w, tab_s],
                tuple(t.float().contiguous() for t in (h2, acc_c, acc_a)),
                dsts, y_buf, route_buf)

    results = []
    for i in range(S):
        out_s = list(st[i]["out_samples"])
        out_c = list(st[i]["out_scores"])
        out_a = list(st[i]["out_alphas"])
        for idx2 in range(st[i]["live"]):
            out_s.append(st[i]["samples"][idx2])
            out_c.append(float(st[i]["scores"][idx2]))
            out_a.append(st[i]["alphas"][idx2])
        results.append((out_s, out_c, out_a))
    if resident:
        _fetch_alignments(results, alog, lens)
    return results


def _fetch_alignments(results, alog, lens):
    """resident_state: replace the (step, batch row) references of every
    hypothesis by the attention rows they name, read from the device log
    ``alog`` (steps, rows, Ts) with one gather and one copy to the host,
    trimmed to the sentence's own length."""
    refs = [ref for _, _, out_a in results for hyp in out_a for ref in hyp]
    if not refs:
        return
    width = alog.shape[1]
    idx = torch.tensor([s * width + r for s, r in refs]).to(alog.device)
    got = alog.reshape(-1, alog.shape[2])[idx].cpu().numpy()
    pos = 0
    for i, (_, _, out_a) in enumerate(results):
        for h, hyp in enumerate(out_a):
            out_a[h] = [got[pos + t, :lens[i]].copy()
                        for t in range(len(hyp))]
            pos += len(hyp)
