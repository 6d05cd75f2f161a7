"""ARPA bigram / trigram language model: host-side parser + dense table for the beam-search kernel.

Same class surface as the reference's timit/utils/NgramLM.py (LanguageModel :11-90): text ARPA with
TAB-separated fields, log10 -> ln, back-off lookup p(w2|w1) = bigram[w1 w2] or backoff(w1)+unigram(w2),
'UNK' aliased to '<unk>'.  `table()` tabulates get_bi_prob over all (previous class, next class) pairs so
that the device kernel (csrc/decode.hip) does one load per LM query.

With n_gram=3 (the reference accepts the argument and creates an empty `trigrame` dict that nothing fills) the \\3-grams: section
is parsed as well, get_tri_prob is the standard ARPA back-off evaluation p(w2|w0 w1) = trigram[w0 w1 w2] or backoff(w0 w1) + p(w2|w1),
and `table()` is (V+1)^3.  With n_gram=2, the default, a \\3-grams: section is ignored.
"""
import math

import numpy as np

n_grams = ["unigram", "bigram", "trigram", "4gram", "5gram"]


class LanguageModel:
    """Attributes the reference exposes: unigram / bigram dicts token(-pair) -> [ln prob, ln back-off], start / end / unk."""

    _SECTION = {"\\1-grams:": "unigram", "\\2-grams:": "bigram"}
    _SECTION3 = dict(_SECTION, **{"\\3-grams:": "trigrame"})

    def __init__(self, arpa_file=None, n_gram=2, start="<s>", end="</s>", unk="<unk>"):
        self.n_gram, self.start, self.end, self.unk = n_gram, start, end, unk
        self.scale = math.log(10)          # ARPA stores log10; the decoder works in ln
        self.initngrams(arpa_file)

    def initngrams(self, fn):
        """Parse the \\1-grams: and \\2-grams: sections: 'log10p<TAB>tokens[<TAB>log10 back-off]' per entry; with n_gram=3 the
        \\3-grams: section too, into `trigrame` (the reference's attribute name), and a section of a higher order is skipped.  With
        n_gram=2 the parser is the one it was: it knows two headers, and whatever follows the bigrams lands in `bigram` under
        keys of three tokens and more, which no lookup forms."""
        self.unigram, self.bigram = {}, {}
        sections = self._SECTION
        if self.n_gram == 3:
            self.trigrame = {}
            sections = self._SECTION3
        target = None
        with open(fn, "r") as f:           # open(None) raises TypeError exactly as in the reference (an LM is mandatory)
            for raw in f:
                line = raw.rstrip("\n")
                if line in sections:
                    target = getattr(self, sections[line])
                    continue
                if self.n_gram == 3 and line.startswith("\\") and line.endswith("-grams:"):
                    target = None
                    continue
                if target is None:
                    continue
                parts = line.split("\t")
                if len(parts) in (2, 3):
                    backoff = self.scale * float(parts[2]) if len(parts) == 3 else 0.0
                    target[parts[1]] = [self.scale * float(parts[0]), backoff]
        self.unigram["UNK"] = self.unigram[self.unk]

    def get_uni_prob(self, wid):
        return self.unigram[wid][0]

    def get_bi_prob(self, w1, w2):
        """ln p(w2 | w1) with back-off; '' stands for sentence start (w1) / end (w2)."""
        prev, nxt = w1 or self.start, w2 or self.end
        hit = self.bigram.get(prev + " " + nxt)
        if hit is not None:
            return hit[0]
        return self.unigram[prev][1] + self.unigram[nxt][0]      # KeyError for a phone missing from the ARPA, as the reference

    def get_tri_prob(self, w0, w1, w2):
        """ln p(w2 | w0 w1) with back-off (n_gram=3); '' stands for sentence start (w0, w1) / end (w2)."""
        a, b, c = w0 or self.start, w1 or self.start, w2 or self.end
        hit = self.trigrame.get(a + " " + b + " " + c)
        if hit is not None:
            return hit[0]
        bo = self.bigram.get(a + " " + b)
        return (bo[1] if bo is not None else 0.0) + self.get_bi_prob(w1, w2)

    def score_tg(self, sentence):
        """ln p of the sentence under the order-3 model: p(w1 | <s>) by get_bi_prob, then get_tri_prob with '<s> w1' as the first context."""
        words = sentence.strip().split()
        if not words:
            raise IndexError("score_tg: empty sentence")
        chain = [self.start] + words + [self.end]
        total = self.get_bi_prob(chain[0], chain[1])
        return float(total + sum(self.get_tri_prob(a, b, c) for a, b, c in zip(chain[:-2], chain[1:-1], chain[2:])))

    def score_bg(self, sentence):
        words = sentence.strip().split()
        if not words:
            raise IndexError("score_bg: empty sentence")         # the reference indexes words[0]
        chain = [self.start] + words + [self.end]
        return float(sum(self.get_bi_prob(a, b) for a, b in zip(chain[:-1], chain[1:])))

    def table(self, classes, blank_index=0):
        """(V+1)x(V+1) float64: [c1][c2] = get_bi_prob(classes[c1], classes[c2]); row V = '<s>', column V = '</s>'.
        The blank class is never queried by the decoder (NaN there)."""
        V = len(classes)
        names = [classes[c] for c in range(V)] + [""]
        live = [c for c in range(V + 1) if c != blank_index]
        tab = np.full((V + 1, V + 1), np.nan, dtype=np.float64)
        for c1 in live:
            tab[c1, live] = [self.get_bi_prob(names[c1], names[c2]) for c2 in live]
        if self.n_gram == 3:
            return self._table3(names, live, tab)
        return tab

    def _table3(self, names, live, bi):
        """(V+1)^3 float64: [c0][c1][k] = ln p(k | c0 c1); index V = '<s>' for c0 and c1, '</s>' for k.  [V][V][k] = p(k | <s>) (the
        bigram row of '<s>'), [V][c1][k] the context of a one-class labelling.  What the decoder never asks for stays NaN: any index
        equal to the blank, and c1 == V ('<s>' behind a class) with c0 != V."""
        V = len(names) - 1
        tab = np.full((V + 1, V + 1, V + 1), np.nan, dtype=np.float64)
        tab[V, V] = bi[V]
        for c0 in live:
            for c1 in live:
                if c1 == V:
                    continue
                key, row = (names[c0] or self.start) + " " + names[c1] + " ", bi[c1]
                hit = self.bigram.get((names[c0] or self.start) + " " + names[c1])
                bo = hit[1] if hit is not None else 0.0
                for k in live:
                    tg = self.trigrame.get(key + (names[k] or self.end))
                    tab[c0, c1, k] = tg[0] if tg is not None else bo + row[k]
        return tab
