"""aws-chunked bodies (STREAMING-AWS4-HMAC-SHA256-PAYLOAD and ...-PAYLOAD-TRAILER) from the rule
alone, in plain Python (bytes, %x, base64): the reference of the body tests, independent of the
library's text functions.

    body = { hex(k) ";chunk-signature=" hex(sig) "\\r\\n" <k bytes> "\\r\\n" }   per data chunk
           "0;chunk-signature=" hex(sig_last) "\\r\\n"
           "\\r\\n"  |  name ":" base64(value) "\\r\\nx-amz-trailer-signature:" hex(sig) "\\r\\n\\r\\n"

`frame` builds bodies; `parse` is a strict decoder written on its own (a state walk over the
bytes, not the inverse of `frame`'s code) that rejects anything malformed.
"""
import base64
import functools
import re

import numpy as np

NAMES = {k: "x-amz-checksum-" + k for k in ("crc32c", "crc32", "crc64nvme", "sha1", "sha256")}
VALUE_BYTES = {"crc32c": 4, "crc32": 4, "crc64nvme": 8, "sha1": 20, "sha256": 32}


def _rows(a, what):
    """Signatures given as (rows, 8) words, or as 32-byte strings -> list of 32-byte strings."""
    if isinstance(a, np.ndarray):
        raw = np.ascontiguousarray(a).tobytes()
        assert len(raw) % 32 == 0, what
        return [raw[i:i + 32] for i in range(0, len(raw), 32)]
    return [bytes(x) for x in a]


def hexlen(k: int) -> int:
    return len("%x" % k)


def body_length(length: int, chunk_bytes: int, kind=None) -> int:
    """The wire length by the rule's arithmetic (not len(frame(...)): the tests compare the two)."""
    full, rem = divmod(length, chunk_bytes)
    ending = 2 if kind is None else len(NAMES[kind]) + 1 + 4 * ((VALUE_BYTES[kind] + 2) // 3) + 94
    return full * (hexlen(chunk_bytes) + 85 + chunk_bytes) + (hexlen(rem) + 85 + rem if rem else 0) + 84 + ending


def frame(parts, chunk_bytes, signatures, kind=None, values=None, trailer_sigs=None):
    """One body (bytes) per part.  `signatures`: part-major, each part's data chunks and its final
    chunk's; `values`: the checksum's header bytes per part (big-endian for the CRCs);
    `trailer_sigs`: one signature per part."""
    sigs = _rows(signatures, "signatures")
    tsigs = None if kind is None else _rows(trailer_sigs, "trailer signatures")
    out, row = [], 0
    for p, part in enumerate(parts):
        part = bytes(part)
        body = []
        for at in range(0, len(part), chunk_bytes):
            chunk = part[at:at + chunk_bytes]
            body += [b"%x;chunk-signature=%s\r\n" % (len(chunk), sigs[row].hex().encode()), chunk, b"\r\n"]
            row += 1
        body.append(b"0;chunk-signature=%s\r\n" % sigs[row].hex().encode())
        row += 1
        if kind is None:
            body.append(b"\r\n")
        else:
            assert len(values[p]) == VALUE_BYTES[kind]
            body.append(NAMES[kind].encode() + b":" + base64.b64encode(bytes(values[p])) + b"\r\n")
            body.append(b"x-amz-trailer-signature:" + tsigs[p].hex().encode() + b"\r\n\r\n")
        out.append(b"".join(body))
    assert row == len(sigs), "signature rows left over"
    return out


_HEAD = re.compile(rb"(0|[1-9a-f][0-9a-f]*);chunk-signature=([0-9a-f]{64})\r\n")
_TRAILER = re.compile(rb"([a-z0-9-]+):([A-Za-z0-9+/]+={0,2})\r\nx-amz-trailer-signature:([0-9a-f]{64})\r\n\r\n")


def parse(body: bytes) -> dict:
    """Decode one body: {"chunks": [bytes], "signatures": [hex str] (one per data chunk, then the
    final chunk's), "trailer_line": "name:base64" or None, "trailer_signature": hex str or None}.
    ValueError for anything that is not exactly a body."""
    body = bytes(body)
    at, chunks, sigs = 0, [], []
    while True:
        m = _HEAD.match(body, at)
        if not m:
            raise ValueError(f"no chunk header at byte {at}")
        k = int(m.group(1), 16)
        sigs.append(m.group(2).decode())
        at = m.end()
        if k == 0:
            break
        if body[at + k:at + k + 2] != b"\r\n" or len(body) < at + k + 2:
            raise ValueError(f"chunk of {k} bytes at byte {at} is not closed by CRLF")
        chunks.append(body[at:at + k])
        at += k + 2
    if body[at:] == b"\r\n":
        return {"chunks": chunks, "signatures": sigs, "trailer_line": None, "trailer_signature": None}
    m = _TRAILER.fullmatch(body, at)
    if not m:
        raise ValueError(f"neither CRLF nor a trailer at byte {at}")
    base64.b64decode(m.group(2), validate=True)
    return {"chunks": chunks, "signatures": sigs,
            "trailer_line": (m.group(1) + b":" + m.group(2)).decode(),
            "trailer_signature": m.group(3).decode()}


# ---- the grid the CPU and the GPU tests share: every chunk size around a change of the length's
# hex digits or of a 16-byte line, each with parts around its multiples
CHUNK_BYTES = (1, 15, 16, 17, 255, 256, 4095, 4096, 65535, 65536, 65537)
KINDS = (None,) + tuple(NAMES)


def grid_lengths(c):
    return [0, 1, c - 1, c, c + 1, 2 * c, 2 * c + 1]


@functools.lru_cache(maxsize=None)
def grid_parts(c):
    """The seven parts of chunk size c (random bytes)."""
    rng = np.random.default_rng(c)
    return tuple(rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in grid_lengths(c))


def random_inputs(rng, parts, c, kind):
    """What the assembler only renders, drawn at random: (rows, 8) signature words, the checksum's
    header bytes per part and (n, 8) trailer signature words (None, None without a kind)."""
    rows = sum(-(-len(p) // c) + 1 for p in parts)
    sigs = rng.integers(0, 2**32, (rows, 8), dtype=np.uint32)
    if kind is None:
        return sigs, None, None
    values = [rng.integers(0, 256, VALUE_BYTES[kind], dtype=np.uint8).tobytes() for _ in parts]
    return sigs, values, rng.integers(0, 2**32, (len(parts), 8), dtype=np.uint32)


@functools.lru_cache(maxsize=None)
def grid_case(c, kind):
    """Random inputs for grid_parts(c) and the reference bodies: (sigs, values, tsigs, bodies)."""
    parts = grid_parts(c)
    sigs, values, tsigs = random_inputs(np.random.default_rng([c, KINDS.index(kind)]), parts, c, kind)
    return sigs, values, tsigs, tuple(frame(parts, c, sigs, kind, values, tsigs))
