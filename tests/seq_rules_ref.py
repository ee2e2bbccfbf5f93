"""Plain-Python restatement of the sequence rules of the mmu decode ("Sequence rules"; include/showo_hip.h): which tokens a
history bans for the next pick, and where a list of produced tokens ends."""


def banned(hist, V, n=0, bad=(), ctx_len=0, min_new=0, eot=-1):
    """the set of tokens in [0, V) that the history `hist` (context ids, then the produced tokens) bans for the next pick:
    n >= 1: every h[j+n-1] whose n - 1 predecessors equal the last n - 1 tokens; every last token of a sequence of `bad` (length >= 2)
    whose other tokens are the end of the history; `eot` while fewer than `min_new` tokens follow the `ctx_len` context ids.
    Ids compare as plain integers; an id outside [0, V) is never banned."""
    h = [int(t) for t in hist]
    ln = len(h)
    out = set()
    if n >= 1 and ln >= n:
        tail = h[ln - n + 1:] if n > 1 else []
        for j in range(0, ln - n + 1):
            if h[j:j + n - 1] == tail:
                out.add(h[j + n - 1])
    for s in bad:
        s = [int(t) for t in s]
        m = len(s)
        if m >= 2 and ln >= m - 1 and h[ln - (m - 1):] == s[:-1]:
            out.add(s[-1])
    if eot >= 0 and ln - ctx_len < min_new:
        out.add(int(eot))
    return {w for w in out if 0 <= w < V}


def stop_cut(tokens, stops, eot=None):
    """`tokens` cut behind the first position at which they end: the token there is `eot`, or the tokens up to it end with one of the
    sequences of `stops`; all of them when they never end"""
    toks = [int(t) for t in tokens]
    for i in range(len(toks)):
        if eot is not None and toks[i] == eot:
            return toks[:i + 1]
        for s in stops or ():
            s = [int(t) for t in s]
            if len(s) <= i + 1 and toks[i + 1 - len(s):i + 1] == s:
                return toks[:i + 1]
    return toks


def table_of(bad):
    """the flat int32 bad-word table of include/showo_hip.h as a list: count, count + 1 offsets, the tokens"""
    off = [0]
    for s in bad:
        off.append(off[-1] + len(s))
    return [len(bad)] + off + [int(t) for s in bad for t in s]


def greedy(bias, steps, V, n=0, bad=(), context=(), min_new=0, eot=-1, stops=()):
    """the greedy answer of a model whose logits are the bias alone ({id: value}, everything else far below): what the path tests
    expect when the bias dominates the tiny model's logits.  It ends early where every biased id is banned: from there on the model's
    own logits decide."""
    hist, out = list(context), []
    for _ in range(steps):
        ban = banned(hist, V, n, bad, len(context), min_new, eot)
        if all(w in ban for w in bias):
            break
        t = max((w for w in bias if w not in ban), key=lambda w: bias[w])
        out.append(t)
        hist.append(t)
        if t == eot or any(len(s) <= len(out) and out[-len(s):] == [int(q) for q in s] for s in stops):
            break
    return out
