"""Host references of the beam search ("Beam search"; csrc/beam.hip).

    select_ref        the selection kernel's arithmetic restated in numpy float32: given the device's (mx, logS) per row it reproduces every
                      score bit and the whole selection
    beam_bookkeeping  the rule of a search -- candidates walked in order, <eot> of rank < B finishes, the B best hypotheses kept, done,
                      the live beams joining at max_new -- over any `pick`: the fp64 reference and the by-hand GPU search share it
    beam_search_ref   the search in numpy float64 over a `logits_of(prefix)` callable
"""
import numpy as np


def select_ref(X, cum, norm, B):
    """X fp32 [nb, V], cum fp32 [nb], norm fp32 [nb, 2] = (mx, logS) -> (score fp32 [2B], beam int32 [2B], token int32 [2B]).
    score = cum[b] + ((x - mx) - logS) in this fp32 order; order (score descending, beam ascending, token ascending); a row whose logS
    is NaN gives (NaN, -1) candidates that come behind every other row's, in (beam, rank) order."""
    X = np.asarray(X, dtype=np.float32)
    cum = np.asarray(cum, dtype=np.float32)
    norm = np.asarray(norm, dtype=np.float32)
    nb, V = X.shape
    K = 2 * B
    bad = np.isnan(norm[:, 1])
    with np.errstate(invalid="ignore", over="ignore"):
        S = (cum[:, None] + ((X - norm[:, 0:1]) - norm[:, 1:2])).astype(np.float32)
    beams = np.repeat(np.arange(nb, dtype=np.int32), V).reshape(nb, V)
    toks = np.tile(np.arange(V, dtype=np.int32), nb).reshape(nb, V)
    good = ~bad
    s, b, t = S[good].reshape(-1), beams[good].reshape(-1), toks[good].reshape(-1)
    if s.size > K:  # the K-th largest score bounds the candidates
        thr = np.partition(s, s.size - K)[s.size - K]
        keep = s >= thr
        s, b, t = s[keep], b[keep], t[keep]
    with np.errstate(invalid="ignore"):
        order = np.lexsort((t, b, -s.astype(np.float64)))[:K]
    score, beam, token = list(s[order]), list(b[order]), list(t[order])
    for r in np.nonzero(bad)[0]:
        for _ in range(K):
            if len(score) < K:
                score.append(np.float32("nan")); beam.append(r); token.append(-1)
    return np.array(score, dtype=np.float32), np.array(beam, dtype=np.int32), np.array(token, dtype=np.int32)


def beam_bookkeeping(pick, B, max_new, eot, final_of, early_stopping):
    """The search over `pick(t, prefixes, cum) -> [(score, beam, token)] * 2B` (sorted; t = 0: one prefix (), cum [0]; later B prefixes)
    and `final_of(score, len)`.  Returns a dict: `hyps` (best first: tokens, final, sumlp, len, step, beam, kind, order), `parent` /
    `token` / `cum` (one list per step taken), `done_step` (generated length at which done was set), `finished_early` (hypotheses that
    ended on <eot>), `dropped` (<eot> candidates of rank >= B), `last_step_eot` (an <eot> of rank < B in the step that reaches
    max_new: the corner in which Hugging Face's bookkeeping differs)."""
    hyps, order = [], 0
    trace = {"parent": [], "token": [], "cum": [], "cands": []}
    prefixes, cum = [()], [0.0]
    stats = {"finished_early": 0, "dropped": 0, "last_step_eot": False, "done_step": None}

    def insert(h):
        nonlocal order
        h["order"] = order
        order += 1
        if len(hyps) == B:
            if not h["final"] > hyps[-1]["final"]:
                return
            hyps.pop()
        i = len(hyps)
        while i > 0 and hyps[i - 1]["final"] < h["final"]:
            i -= 1
        hyps.insert(i, h)

    for t in range(max_new):
        length = t + 1
        cands = pick(t, prefixes, cum)
        trace["cands"].append(cands)
        live = []
        for r, (s, b, tk) in enumerate(cands[:2 * B]):
            if eot is not None and tk == eot:
                if r < B:
                    insert({"tokens": list(prefixes[b]) + [tk], "final": final_of(s, length), "sumlp": s, "len": length, "step": t,
                            "beam": int(b), "kind": 0})
                    stats["finished_early"] += 1
                    stats["last_step_eot"] |= length == max_new
                else:
                    stats["dropped"] += 1
            elif len(live) < B:
                live.append((s, int(b), int(tk)))
        assert len(live) == B
        trace["parent"].append([b for _, b, _ in live])
        trace["token"].append([tk for _, _, tk in live])
        trace["cum"].append([s for s, _, _ in live])
        prefixes = [tuple(prefixes[b]) + (tk,) for _, b, tk in live]
        cum = [s for s, _, _ in live]
        done = len(hyps) == B and (early_stopping or hyps[-1]["final"] >= final_of(cum[0], length))
        if not done and length == max_new:
            for b in range(B):
                insert({"tokens": list(prefixes[b]), "final": final_of(cum[b], length), "sumlp": cum[b], "len": length, "step": t,
                        "beam": b, "kind": 1})
            done = True
        if done:
            stats["done_step"] = length
            break
    return dict(hyps=hyps, **trace, **stats)


def beam_search_ref(logits_of, B, max_new, eot, length_penalty, early_stopping):
    """beam search in numpy float64.  logits_of(prefix tuple) -> the logits row behind the prompt + prefix.  Besides beam_bookkeeping's
    fields: `gap`, the smallest difference between neighbours among the first 2B + 1 candidates (so also between candidate 2B and
    candidate 2B + 1) over the steps taken."""
    gaps = []

    def pick(t, prefixes, cum):
        rows = []
        for b, p in enumerate(prefixes):
            x = np.asarray(logits_of(tuple(p)), dtype=np.float64).reshape(-1)
            m = x.max()
            lp = x - m - np.log(np.exp(x - m).sum())
            rows.append(cum[b] + lp)
        S = np.stack(rows)
        nb, V = S.shape
        flat = S.reshape(-1)
        order = np.lexsort((np.tile(np.arange(V), nb), np.repeat(np.arange(nb), V), -flat))[:2 * B + 1]
        if len(order) > 2 * B:  # (the smallest step among the first 2B + 1: the order INSIDE the 2B decides ranks and beam indices too)
            gaps.append(float(np.min(-np.diff(flat[order]))))
        return [(float(flat[i]), int(i // V), int(i % V)) for i in order[:2 * B]]

    out = beam_bookkeeping(pick, B, max_new, eot, lambda s, n: s / float(n) ** float(length_penalty), early_stopping)
    out["gap"] = min(gaps) if gaps else float("inf")
    return out
