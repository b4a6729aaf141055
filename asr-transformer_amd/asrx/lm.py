"""Back-off n-gram language models over the model's own token ids, for shallow fusion in beam search and for
second-pass rescoring (asrx_ngram_score / asrx_ngram_advance / asrx_ngram_seq_logprob, include/asrx.h).

An NgramLM is built on the host from {token tuple: (logp, backoff)} in natural-log units (or parsed from an ARPA
file, or estimated from token sequences) and laid out as the forward trie in breadth-first order that the kernels
walk: node 0 the empty context, nodes 1 .. V the unigrams (dense: token v is node 1 + v), higher orders level by
level, the children of a node contiguous and sorted by token.  `.to(device)` puts the four arrays on the device."""
import math
import os
from collections import defaultdict

import torch

from ._lib import NGRAM_MAX_ORDER

INF = float("inf")
LN10 = math.log(10.0)


class NgramLM:
    """ngrams: {tuple of 1 .. order token ids: (logp, backoff)}, natural log; backoff None or 0 where the model gives
    none.  Every n-gram of two or more tokens needs its prefix (the tuple without its last token) among the keys,
    else ValueError.  Unigrams that are not given carry `oov_logp` and no back-off weight.  bos_id: the
    sentence-start token the decoders put in front of every hypothesis (None: none)."""

    def __init__(self, ngrams, order, vocab_size, bos_id=1, oov_logp=-INF, eos_id=None):
        order, V = int(order), int(vocab_size)
        if not 1 <= order <= NGRAM_MAX_ORDER:
            raise ValueError(f"order must be in 1..{NGRAM_MAX_ORDER}, got {order}")
        if not 1 <= V <= 1 << 20:
            raise ValueError(f"vocab_size must be in 1..2^20, got {vocab_size}")
        if bos_id is not None and not 0 <= int(bos_id) < V:
            raise ValueError(f"bos_id {bos_id} outside the vocabulary [0, {V})")
        oov_logp = float(oov_logp)
        if oov_logp != oov_logp or oov_logp > 0.0:
            raise ValueError(f"oov_logp must be a log-probability, got {oov_logp}")
        self.order, self.vocab_size = order, V
        self.bos_id = None if bos_id is None else int(bos_id)
        self.eos_id = None if eos_id is None else int(eos_id)
        self.oov_logp = oov_logp
        self.dropped = 0
        grams = {}
        for g, (lp, bo) in ngrams.items():
            g = tuple(int(t) for t in g)
            lp, bo = float(lp), 0.0 if bo is None else float(bo)
            if not 1 <= len(g) <= order:
                raise ValueError(f"n-gram {g} has {len(g)} tokens, the order is {order}")
            if any(not 0 <= t < V for t in g):
                raise ValueError(f"n-gram {g} holds a token outside [0, {V})")
            if lp != lp or lp == INF or bo != bo or abs(bo) == INF:
                raise ValueError(f"n-gram {g}: logp {lp} / backoff {bo} is no log-probability / finite weight")
            grams[g] = (lp, bo)
        for g in grams:
            if len(g) > 1 and g[:-1] not in grams:
                raise ValueError(f"n-gram {g} is in the table but its prefix {g[:-1]} is not")
        self.ngrams = grams
        # breadth-first layout: the nodes of each level ordered by (parent node, token)
        node = {(v,): 1 + v for v in range(V)}
        token = [-1] + list(range(V))
        logp = [0.0] + [grams.get((v,), (oov_logp, 0.0))[0] for v in range(V)]
        backoff = [0.0] + [grams.get((v,), (oov_logp, 0.0))[1] for v in range(V)]
        parent_of = [0] * V
        for n in range(2, order + 1):
            level = sorted((g for g in grams if len(g) == n), key=lambda g: (node[g[:-1]], g[-1]))
            for g in level:
                node[g] = len(token)
                token.append(g[-1])
                logp.append(grams[g][0])
                backoff.append(grams[g][1])
                parent_of.append(node[g[:-1]])
        n_nodes = len(token)
        nchild = [0] * n_nodes
        for p in parent_of:
            nchild[p] += 1
        first = [1]
        for i in range(n_nodes):
            first.append(first[-1] + nchild[i])
        assert first[-1] == n_nodes
        self.n_nodes = n_nodes
        self._logp64, self._backoff64, self._first, self._token = logp, backoff, first, token
        self.first_child = torch.tensor(first, dtype=torch.int32)
        self.token = torch.tensor(token, dtype=torch.int32)
        self.logp = torch.tensor(logp, dtype=torch.float64).float()
        self.backoff = torch.tensor(backoff, dtype=torch.float64).float()

    # ------------------------------------------------------------------------------------------ device
    def to(self, device):
        """Move the table to `device` (in place) and return self."""
        for name in ("first_child", "token", "logp", "backoff"):
            setattr(self, name, getattr(self, name).to(device).contiguous())
        return self

    @property
    def device(self):
        return self.logp.device

    def table_args(self):
        """The leading arguments of every asrx_ngram_* entry point."""
        return (self.first_child.data_ptr(), self.token.data_ptr(), self.logp.data_ptr(), self.backoff.data_ptr(),
                self.n_nodes, self.order, self.vocab_size)

    # ------------------------------------------------------------------------------------------ host scorer
    def _child(self, node, tok):
        lo, hi = self._first[node], self._first[node + 1]
        end = hi
        while lo < hi:
            mid = (lo + hi) // 2
            if self._token[mid] < tok:
                lo = mid + 1
            else:
                hi = mid
        return lo if lo < end and self._token[lo] == tok else -1

    def context(self, history):
        """The hypothesis state after `history` (all of it, the sentence start included if there is one): a list of
        order - 1 node numbers, [k - 1] the node spelling the last k tokens or -1."""
        history = [int(t) for t in history]
        out = []
        for k in range(1, self.order):
            nd = -1
            if k <= len(history) and all(0 <= t < self.vocab_size for t in history[-k:]):
                nd = 1 + history[-k]
                for t in history[len(history) - k + 1:]:
                    nd = self._child(nd, t)
                    if nd < 0:
                        break
            out.append(nd)
        return out

    def logprob(self, history, token):
        """log p(token | history) in fp64 on the host, by the kernels' rule: the longest context that has the token,
        plus the back-off weights of every longer context that exists."""
        token = int(token)
        if not 0 <= token < self.vocab_size:
            raise ValueError(f"token {token} outside [0, {self.vocab_size})")
        ctx = self.context(history)
        ks, hit = 0, 1 + token
        for k in range(self.order - 1, 0, -1):
            if ctx[k - 1] >= 0:
                c = self._child(ctx[k - 1], token)
                if c >= 0:
                    ks, hit = k, c
                    break
        acc = self._logp64[hit]
        for j in range(ks + 1, self.order):
            if ctx[j - 1] >= 0:
                acc += self._backoff64[ctx[j - 1]]
        return acc

    # ------------------------------------------------------------------------------------------ ARPA
    @classmethod
    def from_arpa(cls, source, vocab_size, token_id=int, bos_id=1, eos_id=2):
        """Parse an ARPA file: `source` is a path, the text itself (a string with line breaks) or an open text file.
        token_id(word) -> the model's id of a word; a word it raises ValueError / KeyError / TypeError for, or maps
        outside [0, vocab_size), is unmapped: every n-gram that holds one is dropped and counted in `.dropped`.
        <s> and </s> are bos_id and eos_id; <unk> is no token, its unigram sets `oov_logp` (n-grams of higher order
        that hold it are dropped).  log10 values become natural logs.  ValueError for a section whose count differs
        from the header's and for an n-gram whose prefix is not in the file."""
        if hasattr(source, "read"):
            text = source.read()
        elif "\n" in source:
            text = source
        else:
            with open(os.fspath(source), "r", encoding="utf-8") as f:
                text = f.read()
        V = int(vocab_size)

        def ident(word):
            if word == "<s>":
                return bos_id
            if word == "</s>":
                return eos_id
            if word.lower() == "<unk>":
                return None
            try:
                t = token_id(word)
            except (ValueError, KeyError, TypeError):
                return None
            return int(t) if t is not None and 0 <= int(t) < V else None

        counts, grams, seen = {}, {}, defaultdict(int)
        oov, dropped, section, ended = -INF, 0, None, False
        for raw in text.splitlines():
            line = raw.strip()
            if not line:
                continue
            if line.startswith("\\"):
                if line == "\\data\\":
                    section = 0
                elif line == "\\end\\":
                    ended = True
                    break
                elif line.endswith("-grams:"):
                    section = int(line[1:-len("-grams:")])
                    if section not in counts:
                        raise ValueError(f"ARPA: section {line} is not announced in the header")
                else:
                    raise ValueError(f"ARPA: unknown marker {line!r}")
                continue
            if section is None:
                continue            # text in front of \data\
            if section == 0:
                if not line.startswith("ngram "):
                    raise ValueError(f"ARPA: bad header line {line!r}")
                n, c = line[len("ngram "):].split("=")
                counts[int(n)] = int(c)
                continue
            f = line.split()
            if len(f) not in (section + 1, section + 2):
                raise ValueError(f"ARPA: bad {section}-gram line {line!r}")
            seen[section] += 1
            lp = float(f[0]) * LN10
            bo = float(f[section + 1]) * LN10 if len(f) == section + 2 else 0.0
            words = f[1:section + 1]
            if section == 1 and words[0].lower() == "<unk>":
                oov = lp
                continue
            ids = [ident(w) for w in words]
            if any(t is None for t in ids):
                dropped += 1
                continue
            grams[tuple(ids)] = (min(lp, 0.0), bo)
        if not counts or not ended:
            raise ValueError("ARPA: no \\data\\ header or no \\end\\ marker")
        for n, c in counts.items():
            if seen[n] != c:
                raise ValueError(f"ARPA: the header announces {c} {n}-grams, the file holds {seen[n]}")
        lm = cls(grams, max(counts), V, bos_id, oov, eos_id)
        lm.dropped = dropped
        return lm

    def write_arpa(self, path):
        """Write the explicit n-grams as an ARPA file that from_arpa(path, vocab_size, int, bos_id, eos_id) reads
        back: ids as decimal words, bos_id as <s>, eos_id as </s>, a finite oov_logp as <unk>."""
        def word(t):
            return "<s>" if t == self.bos_id else "</s>" if t == self.eos_id else str(t)

        def num(x):
            return "-inf" if x == -INF else repr(x / LN10)

        levels = [sorted(g for g in self.ngrams if len(g) == n) for n in range(1, self.order + 1)]
        unk = self.oov_logp != -INF
        with open(os.fspath(path), "w", encoding="utf-8") as f:
            f.write("\\data\\\n")
            for n, level in enumerate(levels, 1):
                f.write(f"ngram {n}={len(level) + (1 if unk and n == 1 else 0)}\n")
            for n, level in enumerate(levels, 1):
                f.write(f"\n\\{n}-grams:\n")
                if unk and n == 1:
                    f.write(f"{num(self.oov_logp)}\t<unk>\n")
                for g in level:
                    lp, bo = self.ngrams[g]
                    tail = f"\t{num(bo)}" if n < self.order and bo != 0.0 else ""
                    f.write(f"{num(lp)}\t{' '.join(word(t) for t in g)}{tail}\n")
            f.write("\n\\end\\\n")

    # ------------------------------------------------------------------------------------------ estimation
    @classmethod
    def estimate(cls, sequences, order, vocab_size, bos_id=1, eos_id=2, exclude=(), discount=0.75):
        """An n-gram model from token sequences (without BOS / EOS; both are added), by interpolated absolute
        discounting stored in back-off form.  With c(h, w) the count of w after the context h, c(h) their sum and
        types(h) the number of different w:
            p(w | h) = (c(h, w) - D) / c(h) + D * types(h) / c(h) * p(w | h[1:])        for a seen (h, w)
            backoff(h) = D * types(h) / c(h)
        so an unseen w after a seen h gets backoff(h) * p(w | h[1:]), and the explicit entry IS the interpolated
        probability.  The unigrams are interpolated with the uniform distribution over the ids not in `exclude`
        (those get -inf).  Every distribution sums to one exactly (up to fp64 rounding)."""
        order, V, D = int(order), int(vocab_size), float(discount)
        if not 0.0 < D < 1.0:
            raise ValueError(f"discount must be in (0, 1), got {discount}")
        if not 1 <= order <= NGRAM_MAX_ORDER:
            raise ValueError(f"order must be in 1..{NGRAM_MAX_ORDER}, got {order}")
        excluded = {int(t) for t in exclude}
        kept = [v for v in range(V) if v not in excluded]
        if not kept:
            raise ValueError("every id is excluded")
        cnt = [defaultdict(lambda: defaultdict(int)) for _ in range(order)]    # [n - 1][context][word]
        for seq in sequences:
            row = [int(bos_id)] + [int(t) for t in seq] + [int(eos_id)]
            if not 0 <= row[0] < V or any(not 0 <= t < V or t in excluded for t in row[1:]):
                raise ValueError(f"sequence {row} holds an id outside [0, {V}) or an excluded one")
            for i in range(1, len(row)):
                for n in range(1, min(order, i + 1) + 1):
                    cnt[n - 1][tuple(row[i - n + 1:i])][row[i]] += 1
        total = sum(cnt[0][()].values())
        if total == 0:
            raise ValueError("no sequences")
        prob = {}                                           # every explicit n-gram -> probability
        lam0 = D * len(cnt[0][()]) / total
        for v in kept:
            c = cnt[0][()].get(v, 0)
            prob[(v,)] = (c - D) / total * (c > 0) + lam0 / len(kept)
        bo = {}
        for n in range(2, order + 1):
            for h, words in cnt[n - 1].items():
                c_h = sum(words.values())
                bo[h] = D * len(words) / c_h
                for w, c in words.items():
                    lower = prob[h[1:] + (w,)]        # (seen at order n, so seen at order n - 1 too)
                    prob[h + (w,)] = (c - D) / c_h + bo[h] * lower
        grams = {g: (math.log(p), math.log(bo[g]) if g in bo else 0.0) for g, p in prob.items()}
        for h in bo:                # (only an excluded BOS is a context without being an explicit n-gram)
            grams.setdefault(h, (-INF, math.log(bo[h])))
        return cls(grams, order, V, bos_id, -INF, eos_id)
