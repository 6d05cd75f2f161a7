"""NIST CTM files for the decoders' timed output (Decoder.decode_timed): one line per token,

    <utterance> <channel> <start s> <duration s> <token> <confidence>

with fixed decimals (times 3, confidence 4), utterances in the order given, tokens in time order.  The reference writes no such file."""


def write_ctm(fh, utt_ids, timed, frame_shift=0.01, channel="1"):
    """Write the entries of Decoder.decode_timed (`timed`, one per utterance of `utt_ids`; token times in frames of `frame_shift` seconds)
    to the text file `fh`.  A None entry (no hypothesis / no alignment) and an utterance without tokens write no line.  Returns the number
    of lines written."""
    if len(utt_ids) != len(timed):
        raise ValueError("write_ctm: %d utterance ids for %d entries" % (len(utt_ids), len(timed)))
    lines = 0
    for utt, entry in zip(utt_ids, timed):
        if entry is None:
            continue
        for tok in entry[0]:
            phone, start, end, conf = tok[:4]
            fh.write("%s %s %.3f %.3f %s %.4f\n" % (utt, channel, start * frame_shift, (end - start) * frame_shift, phone, conf))
            lines += 1
    return lines


def read_ctm(fh):
    """The inverse of write_ctm: {utterance: [(token, start s, duration s, confidence, channel), ...]} with the utterances in file order
    (a dict keeps it) and the tokens in line order.  Blank lines and ';;' comment lines are skipped; a line without a confidence gets None."""
    out = {}
    for line in fh:
        f = line.split()
        if not f or f[0].startswith(";;"):
            continue
        if len(f) < 5:
            raise ValueError("read_ctm: expected 'utt chan start dur token [conf]', got %r" % line)
        out.setdefault(f[0], []).append((f[4], float(f[2]), float(f[3]), float(f[5]) if len(f) > 5 else None, f[1]))
    return out
