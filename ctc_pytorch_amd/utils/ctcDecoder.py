"""Greedy and beam CTC decoders -- class surface of the reference's timit/utils/ctcDecoder.py
(Decoder :9-149, GreedyDecoder :152-166, BeamDecoder :168-192).

String conversion and CER/WER scoring are host logic (python, as in the reference); the arithmetic --
arg-max over classes, path collapse, prefix beam search -- runs in libctcn.so on the GPU.  `decode`
accepts the CPU tensor the reference hands over (test_ctc.py:85-86) and moves it to the device itself.
"""
import numpy as np
import torch

from ctc_pytorch_amd import ops


def _to_device(t):
    return t if t.is_cuda else t.to("cuda")


class Decoder(object):
    """Host-side string assembly and scoring shared by both decoders (reference class of the same name,
    ctcDecoder.py:9-149): label ids -> phone strings, Levenshtein-based CER / WER, running totals."""

    def __init__(self, int2char, space_idx=1, blank_index=0):
        self.int_to_char, self.space_idx, self.blank_index = int2char, space_idx, blank_index
        self.num_word = self.num_char = 0

    def decode(self):
        raise NotImplementedError

    # ---- scoring ---------------------------------------------------------------------------------------
    @staticmethod
    def _edit_distance(src_seq, tgt_seq):
        """Levenshtein distance (unit costs) of two strings or two lists of hashables (ctcDecoder.py:131-150), in the library's host code
        (ctcn_levenshtein): the reference's interpreter loop over an (L1 + 1) x (L2 + 1) table is seconds per long utterance."""
        n_src, n_tgt = len(src_seq), len(tgt_seq)
        if 0 in (n_src, n_tgt):
            return n_src + n_tgt
        if isinstance(src_seq, str) and isinstance(tgt_seq, str):
            a = np.frombuffer(src_seq.encode("utf-32-le", "surrogatepass"), dtype=np.int32)
            b = np.frombuffer(tgt_seq.encode("utf-32-le", "surrogatepass"), dtype=np.int32)
        else:
            ids = {}
            a = np.asarray([ids.setdefault(t, len(ids)) for t in src_seq], dtype=np.int32)
            b = np.asarray([ids.setdefault(t, len(ids)) for t in tgt_seq], dtype=np.int32)
        from ctc_pytorch_amd import _lib
        d = _lib.lib().ctcn_levenshtein(a.ctypes.data, len(a), b.ctypes.data, len(b))
        if d < 0:
            raise RuntimeError("ctcn_levenshtein failed")
        return int(d)

    def cer(self, s1, s2):
        return self._edit_distance(s1, s2)

    def wer(self, s1, s2):
        a, b = s1.split(), s2.split()
        ids = {}
        for w in a + b:
            ids.setdefault(w, len(ids))
        return self._edit_distance([ids[w] for w in a], [ids[w] for w in b])

    def phone_word_error(self, prob_tensor, frame_seq_len, targets, target_sizes):
        hyps = self.decode(prob_tensor, frame_seq_len)
        refs = self._process_strings(self._convert_to_strings(self._unflatten_targets(targets, target_sizes)))
        char_errs = word_errs = 0
        for hyp, ref in zip(hyps, refs):
            char_errs += self.cer(hyp, ref)
            word_errs += self.wer(hyp, ref)
            self.num_word += len(ref.split())
            self.num_char += len(ref)
        return char_errs, word_errs

    # ---- error breakdown -------------------------------------------------------------------------------
    def _device_ids(self, prob_tensor, frame_seq_len):
        """The decoder's label ids where it produces them: (ids (B, T) int32, lengths (B) int32, status (B) int32 or None), on the device."""
        raise NotImplementedError

    def error_ops(self, prob_tensor, frame_seq_len, targets, target_sizes, class_map=None, stats=None):
        """The error breakdown of one batch (ops.edit_ops on the label ids the decoder leaves on the device; the reference has no counterpart):
        prob_tensor / frame_seq_len as `decode` takes them, targets the padded (B, Lmax) labels of the loader or the concatenated labels
        `phone_word_error` takes (those on the host), class_map the fold of utils.scoring.load_phone_map, stats a utils.scoring.ErrorStats
        that takes the totals and the confusion table.  Returns the six totals (sub, del, ins, cor, hyp_len, ref_len) of the batch: a list
        of ints after ONE device-to-host copy (totals, table and the search's status words in one buffer) -- or, when `stats` accumulates
        on the device, a device tensor and no copy at all (a beam search's status words are then not looked at: an utterance whose search
        failed counts as an empty hypothesis)."""
        ids, ids_len, status = self._device_ids(prob_tensor, frame_seq_len)
        dev = ids.device
        sizes = torch.as_tensor(np.asarray([int(n) for n in target_sizes], dtype=np.int64)) if not torch.is_tensor(target_sizes) else target_sizes
        tg = targets if torch.is_tensor(targets) else torch.as_tensor(np.asarray(targets, dtype=np.int64))
        if tg.dim() != 2:
            rows = self._unflatten_targets(tg.reshape(-1).numpy(), sizes.tolist())
            tg = torch.zeros((len(rows), max([len(r) for r in rows] + [1])), dtype=torch.int64)
            for b, r in enumerate(rows):
                tg[b, :len(r)] = torch.as_tensor(np.asarray(r, dtype=np.int64))
        V = stats.V if stats is not None else None
        on_device = stats is not None and stats.confusion.is_cuda
        table = None
        if stats is not None:
            table = stats.confusion if on_device else torch.zeros((V + 1, V + 1), dtype=torch.int64, device=dev)
        counts = ops.edit_ops(ids, ids_len, tg, sizes, class_map=class_map, num_classes=V, confusion=table).counts
        if on_device:
            tot = counts.sum(0, dtype=torch.int64)
            stats.add(tot)
            return tot
        parts = [counts.sum(0, dtype=torch.int64)] + ([table.reshape(-1)] if table is not None else []) + ([status.to(torch.int64)] if status is not None else [])
        blob = torch.cat(parts).cpu().numpy()
        if status is not None:
            from ctc_pytorch_amd.utils.BeamSearch import ctcBeamSearch
            ctcBeamSearch._checked(None, None, blob[len(blob) - status.numel():])
        if stats is not None:
            stats.add(blob[:6], blob[6:6 + (V + 1) ** 2].reshape(V + 1, V + 1))
        return [int(v) for v in blob[:6]]

    # ---- forced alignment ------------------------------------------------------------------------------
    def align(self, prob_tensor, frame_seq_len, targets, target_sizes, frame_stride=1):
        """Where each label of the KNOWN transcript sits in time (ops.ctc_forced_align: the best CTC path of the transcript; the reference
        has no counterpart -- the capability of torchaudio's forced_align + merge_tokens).  prob_tensor: the (T, B, V) log-prob tensor
        `decode` takes (moved to the device if it is not there); targets / target_sizes: the concatenated labels and sizes `phone_word_error` takes.  Returns one
        entry per utterance: (spans, score) with spans = [(token, start, end, mean frame log-prob over the span), ...] in label order,
        start / end = first and one-past-last frame times frame_stride (the front-end's subsampling: a plain multiplier), score = the
        path's log-probability; None for an utterance that has no alignment.  One device-to-host copy per batch."""
        sizes = [int(n) for n in target_sizes]
        tg = targets if torch.is_tensor(targets) else torch.as_tensor(np.asarray(targets, dtype=np.int64))
        lens = frame_seq_len if torch.is_tensor(frame_seq_len) else [int(n) for n in frame_seq_len]
        a = ops.ctc_forced_align(_to_device(prob_tensor), tg.reshape(-1).to(torch.int64), lens, sizes, blank=self.blank_index)
        B, T = a.paths.shape
        parts = [a.frame_scores, a.scores, a.ok.view(torch.float32), a.starts.view(torch.float32), a.ends.view(torch.float32)]
        blob = torch.cat([p.reshape(-1) for p in parts]).cpu().numpy()
        cuts = np.cumsum([p.numel() for p in parts])[:-1]
        fs, sc, ok, st, en = np.split(blob, cuts)
        rows = self._unflatten_targets(tg.reshape(-1).cpu().numpy(), sizes)
        return self._spans(fs.reshape(B, T), sc, ok.view(np.int32), st.view(np.int32).reshape(B, -1), en.view(np.int32).reshape(B, -1), rows,
                           frame_stride)

    def _spans(self, frame_scores, scores, ok, starts, ends, label_rows, frame_stride=1):
        """Host half of `align`: the arrays of ops.ctc_forced_align (on the host) -> per utterance ([(token, start * frame_stride,
        end * frame_stride, mean of frame_scores[start:end]), ...], score), or None where ok is 0.  No per-frame loop: the means are
        differences of one running sum per utterance (float64)."""
        out = []
        for b, labels in enumerate(label_rows):
            if not ok[b]:
                out.append(None)
                continue
            n = len(labels)
            s, e = starts[b, :n].astype(np.int64), ends[b, :n].astype(np.int64)
            run = np.concatenate([[0.0], np.cumsum(frame_scores[b], dtype=np.float64)])
            mean = (run[e] - run[s]) / np.maximum(e - s, 1)
            spans = [(self.int_to_char[int(labels[j])], int(s[j]) * frame_stride, int(e[j]) * frame_stride, float(mean[j])) for j in range(n)]
            out.append((spans, float(scores[b])))
        return out

    # ---- timed, scored output ----------------------------------------------------------------------------
    def decode_timed(self, prob_tensor, frame_seq_len, frame_stride=1, detail=False):
        """What `decode` recognises, with where and how sure (ops.path_tokens; the reference has no counterpart): one entry per utterance,
        (tokens, score) with tokens = [(phone, start * frame_stride, end * frame_stride, confidence), ...] in time order, start / end = the
        token's first and one-past-last frame, confidence = exp(mean log-prob of the phone over its frames) in (0, 1], score = the
        log-probability of the path the tokens were read from.  detail=True: tokens are (phone, start, end, confidence, min_lp, mean_margin)
        -- the phone's lowest frame log-prob and its mean lead over the best other class.  frame_stride is a plain multiplier, as in
        `align`.  One device-to-host copy per batch."""
        raise NotImplementedError

    def timed_strings(self, timed):
        """The strings `decode` returns for the same batch, from the entries of `decode_timed` (all of them present): each token
        contributes ' ' + phone when space_idx == -1, else the space symbol becomes ' ' (GreedyDecoder.decode's rule; BeamDecoder joins
        the phones with ' ', as its search does)."""
        if self.space_idx == -1:
            return ["".join([" " + tok[0] for tok in entry[0]]) for entry in timed]
        space = self.int_to_char[self.space_idx]
        return ["".join([" " if tok[0] == space else tok[0] for tok in entry[0]]) for entry in timed]

    def _timed(self, pt, frame_stride=1, detail=False, ok=None):
        """Host half of `decode_timed`: an ops.PathTokens (on the device) and, optionally, a (B) int32 device vector `ok` (0: the utterance
        has no entry) -> the list `decode_timed` returns, after one copy of everything to the host."""
        B, T = pt.ids.shape
        f = lambda t: t.reshape(-1).view(torch.float32)
        parts = [f(pt.ids), f(pt.starts), f(pt.ends), f(pt.lengths), pt.mean_lp.reshape(-1), pt.min_lp.reshape(-1), pt.mean_margin.reshape(-1),
                 pt.path_score.reshape(-1)] + ([f(ok.to(torch.int32))] if ok is not None else [])
        blob = torch.cat(parts).cpu().numpy()
        cuts = np.cumsum([p.numel() for p in parts])[:-1]
        ids, st, en, n, mean, mn, mg, sc, *rest = np.split(blob, cuts)
        ids, st, en = (a.view(np.int32).reshape(B, T) for a in (ids, st, en))
        n, mean, mn, mg = n.view(np.int32), mean.reshape(B, T), mn.reshape(B, T), mg.reshape(B, T)
        good = rest[0].view(np.int32) if rest else np.ones(B, dtype=np.int32)
        conf = np.exp(mean.astype(np.float64))
        out = []
        for b in range(B):                                             # (whole rows through tolist(): no per-token numpy scalar)
            if not good[b]:
                out.append(None)
                continue
            k = int(n[b])
            cols = [[self.int_to_char[i] for i in ids[b, :k].tolist()], (st[b, :k] * frame_stride).tolist(), (en[b, :k] * frame_stride).tolist(),
                    conf[b, :k].tolist()] + ([mn[b, :k].tolist(), mg[b, :k].tolist()] if detail else [])
            out.append((list(zip(*cols)), float(sc[b])))
        return out

    # ---- id / string plumbing ----------------------------------------------------------------------------
    @staticmethod
    def _unflatten_targets(targets, target_sizes):
        bounds = np.concatenate([[0], np.cumsum([int(n) for n in target_sizes])])
        return [targets[bounds[i]:bounds[i + 1]] for i in range(len(bounds) - 1)]

    def _convert_to_string(self, seq, sizes):
        symbols = [self.int_to_char[seq[i]] for i in range(sizes)]
        return symbols if self.space_idx == -1 else "".join(symbols)

    def _convert_to_strings(self, seq, sizes=None):
        return [self._convert_to_string(row, len(row) if sizes is None else sizes[k]) for k, row in enumerate(seq)]

    def _process_string(self, seq, remove_rep=False):
        """Drop blanks (and, optionally, frame-to-frame repeats); phones are joined as ' '+phone when the vocabulary
        has no space symbol (space_idx == -1), else the space symbol becomes ' '."""
        blank = self.int_to_char[self.blank_index]
        space = None if self.space_idx == -1 else self.int_to_char[self.space_idx]
        pieces = []
        for pos, sym in enumerate(seq):
            if sym == blank or (remove_rep and pos > 0 and sym == seq[pos - 1]):
                continue
            pieces.append(" " + sym if space is None else (" " if sym == space else sym))
        return "".join(pieces)

    def _process_strings(self, seqs, remove_rep=False):
        return [self._process_string(one, remove_rep) for one in seqs]


class GreedyDecoder(Decoder):
    def decode_ids(self, prob_tensor, frame_seq_len):
        """(T,B,V) log-probs -> list of collapsed id lists (blank and frame-to-frame repeats removed)."""
        lp = _to_device(prob_tensor)
        idx = ops.argmax_last(lp)                                  # (T,B) int32, lowest index on ties
        ids, out_len = ops.greedy_collapse(idx, frame_seq_len, blank=self.blank_index)
        ids_c, len_c = ids.cpu().numpy(), out_len.cpu().numpy()
        return [list(map(int, ids_c[b, : len_c[b]])) for b in range(ids_c.shape[0])]

    def _strings(self, ids_c, len_c):
        """Collapsed ids (B, T) + lengths -> the reference's strings: each kept frame contributes ' ' + phone when space_idx == -1, else the
        space symbol becomes ' ' (ctcDecoder.py:80-92) -- one native pass (ops.join_tokens) over a vocabulary with that already applied."""
        voc = getattr(self, "_voc", None)
        snap = tuple(self.int_to_char.items()) if isinstance(self.int_to_char, dict) else tuple(self.int_to_char)     # (content, not identity: an edited vocabulary must not decode through the old one)
        if voc is None or voc[0] != snap or voc[1] != self.space_idx:
            items = self.int_to_char.items() if isinstance(self.int_to_char, dict) else enumerate(self.int_to_char)
            if self.space_idx == -1:
                words = {k: " " + w for k, w in items}
            else:
                sp = self.int_to_char[self.space_idx]
                words = {k: (" " if w == sp else w) for k, w in items}
            voc = self._voc = (snap, self.space_idx, words)
        return ops.join_tokens(ids_c, len_c, voc[2], "")

    def _device_ids(self, prob_tensor, frame_seq_len):
        ids, out_len = ops.greedy_collapse(ops.argmax_last(_to_device(prob_tensor)), frame_seq_len, blank=self.blank_index)
        return ids, out_len, None

    def decode_timed(self, prob_tensor, frame_seq_len, frame_stride=1, detail=False):
        """Decoder.decode_timed on the arg-max path: the tokens are `decode`'s, a token's frames the run of arg-max frames it was collapsed from."""
        lp = _to_device(prob_tensor)
        return self._timed(ops.path_tokens(ops.argmax_last(lp), frame_seq_len, lp, blank=self.blank_index), frame_stride, detail)

    def decode(self, prob_tensor, frame_seq_len):
        """Same strings as the reference: each kept frame contributes ' '+phone when space_idx == -1."""
        lp = _to_device(prob_tensor)
        idx = ops.argmax_last(lp)
        ids, out_len = ops.greedy_collapse(idx, frame_seq_len, blank=self.blank_index)
        return self._strings(ids.cpu().numpy(), out_len.cpu().numpy())


class BeamDecoder(Decoder):
    def __init__(self, int2char, beam_width=200, blank_index=0, space_idx=-1, lm_path=None, lm_alpha=0.01, lm_order=2, rnnlm=None,
                 rnnlm_weight=0.5, rnnlm_nbest=10, rnnlm_len_bonus=0.0):
        """lm_order: 2 = the reference's bigram search; 3 = the ARPA file's \\3-grams: section joins it (LanguageModel(n_gram=3)).
        rnnlm (an RNNLM or the path of its package; None: every method takes the path it always took): the search returns its rnnlm_nbest
        best labellings (clamped to the beam width), the LM scores them, and the hypothesis is the one with the largest
        (search score + rnnlm_weight * ln P_lm) + rnnlm_len_bonus * length -- n-best rescoring; the search itself does not change."""
        self.beam_width = beam_width
        super().__init__(int2char, space_idx=space_idx, blank_index=blank_index)
        from ctc_pytorch_amd.utils import BeamSearch as uBeam
        from ctc_pytorch_amd.utils import NgramLM as uNgram
        lm = uNgram.LanguageModel(arpa_file=lm_path, n_gram=lm_order)
        self._decoder = uBeam.ctcBeamSearch(int2char, beam_width, lm, lm_alpha=lm_alpha, blank_index=blank_index)
        self.rnnlm = None
        if rnnlm is not None:
            from ctc_pytorch_amd.models.model_rnnlm import RNNLM
            self.rnnlm = rnnlm if isinstance(rnnlm, RNNLM) else RNNLM.load_package(rnnlm)
            if self.rnnlm.num_class != len(int2char):
                raise ValueError("BeamDecoder: the RNN LM has %d classes, the vocabulary %d" % (self.rnnlm.num_class, len(int2char)))
            if int(rnnlm_nbest) < 1:
                raise ValueError("BeamDecoder: rnnlm_nbest must be at least 1")
            self.rnnlm_weight, self.rnnlm_len_bonus = float(rnnlm_weight), float(rnnlm_len_bonus)
            self.rnnlm_nbest = min(int(rnnlm_nbest), int(beam_width))

    def _rescored(self, lp, frame_seq_len):
        """The rescoring pipeline on the current stream: n-best search, one small read of the longest hypothesis, pack, RNNLM forward in
        evaluation mode, log-softmax + NLL, select.  Returns (ops.RescoredBest, status (B)), all on the device.  An utterance whose search
        reports a status has no candidates: its hypothesis is empty."""
        d = self._decoder
        if next(self.rnnlm.parameters()).device != lp.device:
            self.rnnlm.to(lp.device)
        out_ids, out_len, score, count, status = ops.beam_decode_nbest_device(lp, frame_seq_len, d._lm_table_on(lp.device), d.lm_alpha, d.beamWidth,
                                                                              self.rnnlm_nbest, d.blank_index, False)
        count = torch.where(status == 0, count, torch.zeros_like(count))
        Lmax = int(out_len.max())                                       # (the one small read)
        best = ops.rescore_nbest((out_ids, out_len, score, count, status), self.rnnlm.score_packed, self.rnnlm_weight, self.rnnlm_len_bonus, L=Lmax,
                                 boundary=d.blank_index)
        return best, status

    def _rescored_strings_async(self, lp, frame_seq_len):
        """decode() through the rescoring pipeline: the results go to pinned host memory behind it; the callable waits for that copy alone,
        raises what the plain decoder raises from the search's status and joins the strings in native host code."""
        best, status = self._rescored(lp, frame_seq_len)
        B, T = best.ids.shape
        whole = torch.cat([best.ids.reshape(-1), best.lengths, status])
        host = torch.empty(whole.shape, dtype=torch.int32, pin_memory=True)
        host.copy_(whole, non_blocking=True)
        event = torch.cuda.Event()
        event.record(torch.cuda.current_stream(lp.device))
        keep = [whole, best]

        def result():
            event.synchronize()
            keep.clear()
            h = host.numpy()
            ids_c, len_c, st = h[: B * T].reshape(B, T), h[B * T: B * T + B], h[B * T + B:]
            self._decoder._checked(None, None, st)
            return ops.join_tokens(ids_c, len_c, self._decoder.classes, " ")
        return result

    def decode(self, prob_tensor, frame_seq_len=None):
        """prob_tensor (T,B,V) log-probs (CPU or device).  exp() is taken on the device in float32."""
        lp = _to_device(prob_tensor)
        if frame_seq_len is None:
            frame_seq_len = [lp.shape[0]] * lp.shape[1]
        if self.rnnlm is not None:
            return self._rescored_strings_async(lp, frame_seq_len)()
        return self._decoder.decode_strings_async(lp, frame_seq_len, input_is_prob=False)()

    def _device_ids(self, prob_tensor, frame_seq_len=None):
        lp = _to_device(prob_tensor)
        if frame_seq_len is None:
            frame_seq_len = [lp.shape[0]] * lp.shape[1]
        if self.rnnlm is not None:
            best, status = self._rescored(lp, frame_seq_len)
            return best.ids, best.lengths, status
        d = self._decoder
        ids, out_len, _, status = ops.beam_decode_device(lp, frame_seq_len, d._lm_table_on(lp.device), d.lm_alpha, d.beamWidth, d.blank_index, False)
        return ids, out_len, status

    def decode_timed(self, prob_tensor, frame_seq_len=None, frame_stride=1, detail=False):
        """Decoder.decode_timed for the search's hypothesis: the hypothesis (the ids the search leaves on the device) is force-aligned to the
        log-probs (ops.ctc_forced_align) and the tokens are read from the alignment's path, so a token's frames are those of its best CTC
        path and `score` is that path's log-probability (not the search's LM-weighted score).  One small read of the hypothesis lengths
        sizes the alignment's lattice (Lmax = the longest hypothesis, not T).  None for an utterance whose search did not end with status 0
        or whose hypothesis has no alignment; a hypothesis beyond the aligner's 2 047 labels raises ValueError."""
        lp = _to_device(prob_tensor)
        if frame_seq_len is None:
            frame_seq_len = [lp.shape[0]] * lp.shape[1]
        ids, out_len, status = self._device_ids(lp, frame_seq_len)
        done = status == 0
        hyp_len = torch.where(done, out_len, torch.zeros_like(out_len)).to(torch.int64)
        Lmax = int(hyp_len.max())                                       # (the one small read)
        if Lmax > 2047:
            raise ValueError("BeamDecoder.decode_timed: a hypothesis of %d labels is beyond the aligner's 2047" % Lmax)
        lens = frame_seq_len if torch.is_tensor(frame_seq_len) else [int(n) for n in frame_seq_len]
        a = ops.ctc_forced_align(lp, ids[:, :Lmax].to(torch.int64), lens, hyp_len, blank=self.blank_index)
        pt = ops.path_tokens(a.paths, lens, lp, blank=self.blank_index, batch_major=True)
        return self._timed(pt, frame_stride, detail, ok=a.ok * done.to(torch.int32))

    def timed_strings(self, timed):
        return [" ".join([tok[0] for tok in entry[0]]) for entry in timed]

    def decode_async(self, prob_tensor, frame_seq_len=None):
        """decode() enqueued on the current stream: returns a callable that waits for this batch alone and returns its strings
        (steps/test_ctc.decode_and_score keeps three batches in flight on three streams: a batch of <= 128 utterances occupies at most
        half of the device for as long as its longest utterance lasts, and the host-side string assembly and scoring of one batch overlaps
        with the search of the next)."""
        lp = _to_device(prob_tensor)
        if frame_seq_len is None:
            frame_seq_len = [lp.shape[0]] * lp.shape[1]
        if self.rnnlm is not None:                    # (the pipeline reads the longest hypothesis once: it is enqueued up to the result copy)
            return self._rescored_strings_async(lp, frame_seq_len)
        return self._decoder.decode_strings_async(lp, frame_seq_len, input_is_prob=False)      # (strings assembled in native host code)
