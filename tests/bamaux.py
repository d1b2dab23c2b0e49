"""Test infrastructure: alignment records WITH auxiliary fields (SAM spec 4.2.4) on top of tests/bamutil.py's record and BGZF
writers, for the loader's BX rule (include/quilt_amd_io.h).  Nothing in the product imports this.

An alignment is bamutil's dict plus ``aux``: a list of ``(tag, type, value)`` -- types ``A c C s S i I f Z H`` with a plain
value, ``B`` with ``(subtype, [values])``; and optionally ``placeholder=True``: the record carries the long-CIGAR form of SAM
spec 4.2.2 (``<l_seq>S<reference length>N`` in the CIGAR field, the dict's own CIGAR as ``CG:B,I`` in front of ``aux``)."""
import struct

from tests import bamutil

_FMT = {"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I", "f": "<f"}


def aux_bytes(fields) -> bytes:
    out = b""
    for tag, ty, val in fields:
        out += tag.encode() + ty.encode()
        if ty == "A":
            out += val.encode()
        elif ty in _FMT:
            out += struct.pack(_FMT[ty], val)
        elif ty in "ZH":
            out += val.encode() + b"\0"
        elif ty == "B":
            sub, vals = val
            out += sub.encode() + struct.pack("<I", len(vals)) + b"".join(struct.pack(_FMT[sub], v) for v in vals)
        else:
            raise ValueError(ty)
    return out


def record(a, cut_aux=None) -> bytes:
    """One BAM record (with its block_size); ``cut_aux``: only that many bytes of the auxiliary data are kept -- the record ends
    inside a field, and its block_size says so."""
    cigar, fields = a["cigar"], list(a.get("aux", []))
    if a.get("placeholder"):
        ref_len = sum(n for n, op in cigar if op in "MDN=X")
        fields = [("CG", "B", ("I", [(n << 4) | bamutil._CIG[op] for n, op in cigar]))] + fields
        cigar = [(len(a["seq"]), "S"), (ref_len, "N")]
    rec = bamutil._record(a["ref_id"], a["pos"] - 1, a["name"], a["mapq"], a["flag"], cigar, a["seq"], a["qual"], tlen=a.get("tlen", 0))
    aux = aux_bytes(fields)
    if cut_aux is not None:
        aux = aux[:cut_aux]
    body = rec[4:] + aux
    return struct.pack("<i", len(body)) + body


def header(refs, sorted_header=True) -> bytes:
    text = ("@HD\tVN:1.6\tSO:%s\n" % ("coordinate" if sorted_header else "unsorted") +
            "".join(f"@SQ\tSN:{n}\tLN:{l}\n" for n, l in refs)).encode()
    data = b"BAM\1" + struct.pack("<i", len(text)) + text + struct.pack("<i", len(refs))
    for n, l in refs:
        nb = n.encode() + b"\0"
        data += struct.pack("<i", len(nb)) + nb + struct.pack("<i", l)
    return data


def write_bam(path, refs, alignments, sorted_header=True, cut_last_aux=None, block=0xff00):
    recs = [record(a) for a in alignments]
    if cut_last_aux is not None:
        recs[-1] = record(alignments[-1], cut_aux=cut_last_aux)
    raw = header(refs, sorted_header) + b"".join(recs)
    with open(path, "wb") as f:
        f.write(b"".join(bamutil.bgzf_block(raw[i:i + block]) for i in range(0, len(raw), block)) + bamutil.bgzf_block(b""))


def last_record_aux(raw: bytes):
    """(offset of the last record's block_size, offset of its auxiliary data, end) in a decompressed BAM stream; None when the
    stream holds no alignment."""
    l_text, = struct.unpack_from("<i", raw, 4)
    p = 8 + l_text
    n_ref, = struct.unpack_from("<i", raw, p)
    p += 4
    for _ in range(n_ref):
        l_name, = struct.unpack_from("<i", raw, p)
        p += 4 + l_name + 4
    last = None
    while p < len(raw):
        size, = struct.unpack_from("<i", raw, p)
        last = p
        p += 4 + size
    if last is None:
        return None
    size, = struct.unpack_from("<i", raw, last)
    l_name, n_cig, l_seq = raw[last + 12], struct.unpack_from("<H", raw, last + 16)[0], struct.unpack_from("<i", raw, last + 20)[0]
    aux = last + 4 + 32 + l_name + 4 * n_cig + (l_seq + 1) // 2 + l_seq
    return last, aux, last + 4 + size


def cut_copies(path, out_prefix, block=0xff00):
    """Copies of the BAM at `path` whose LAST record is cut at every byte of its auxiliary data (block_size adjusted: the record
    ends inside a field).  Returns the paths written."""
    raw = bamutil.bgzf_decompress(open(path, "rb").read())
    where = last_record_aux(raw)
    out = []
    if where is None:
        return out
    last, aux, end = where
    for keep in range(aux, end):
        body = raw[last + 4:keep]
        data = raw[:last] + struct.pack("<i", len(body)) + body
        p = f"{out_prefix}.cut{keep - aux}.bam"
        with open(p, "wb") as f:
            f.write(b"".join(bamutil.bgzf_block(data[i:i + block]) for i in range(0, len(data), block)) + bamutil.bgzf_block(b""))
        out.append(p)
    return out
