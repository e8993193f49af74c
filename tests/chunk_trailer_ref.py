"""SigV4 trailer signatures (STREAMING-AWS4-HMAC-SHA256-PAYLOAD-TRAILER) from hashlib + hmac +
base64 alone, on top of tests/chunk_sign_ref.py: the reference of the trailer tests, independent
of the library.

    line        = name ":" base64(value) "\\n"
    trailer_sig = HMAC-SHA256(signing_key, "AWS4-HMAC-SHA256-TRAILER\\n" timestamp "\\n"
                    date/region/service/aws4_request "\\n" hex(last chunk signature) "\\n"
                    hex(sha256(line)))

CRC references: zlib.crc32, and bitwise table code for CRC-32C and CRC-64/NVME.
"""
import base64
import hashlib
import zlib

import numpy as np

from tests import chunk_sign_ref as ref

KINDS = ("crc32c", "crc32", "crc64nvme", "sha1", "sha256")
CRC_KINDS = KINDS[:3]
NAMES = {k: "x-amz-checksum-" + k for k in KINDS}
# the known answer: 66,560 x 'a' at 65,536-byte chunks in chunk_sign_ref's setting, seeded with
# the signature of the trailer form's request headers
KNOWN_SEED = "106e2a8a18243abcf37539882f36619c00e2dfc72633413f02d3b74544bfeb8e"
KNOWN_SIGNATURES = ("b474d8862b1487a5145d686f57f013e54db672cee1c953b3010fb58501ef5aa2",
                    "1c1344b170168f8e65b41376b44b20fe354e373826ccbbe2c1d40a8cae51e5c7",
                    "2ca2aba2005185cf7159c6277faf83795951dd77a3a99e6e65d5c9f85863f992")
KNOWN_LINE = "x-amz-checksum-crc32c:sOO8/Q=="
KNOWN_TRAILER_SIGNATURE = "d81f82fc3505edab99d459891051a732e8730629a2e4a59689829ca17fe2e435"


def _table(poly: int) -> list[int]:
    """Byte table of a reflected CRC, bit by bit from the reflected polynomial."""
    t = []
    for b in range(256):
        v = b
        for _ in range(8):
            v = (v >> 1) ^ (poly if v & 1 else 0)
        t.append(v)
    return t


_T32C = _table(0x82F63B78)
_T64 = _table(0x9A6C9329AC4BC9B5)


def crc32c(data: bytes) -> int:
    v = 0xFFFFFFFF
    for b in data:
        v = (v >> 8) ^ _T32C[(v ^ b) & 255]
    return v ^ 0xFFFFFFFF


def crc64nvme(data: bytes) -> int:
    v = 0xFFFFFFFFFFFFFFFF
    for b in data:
        v = (v >> 8) ^ _T64[(v ^ b) & 255]
    return v ^ 0xFFFFFFFFFFFFFFFF


assert crc32c(b"123456789") == 0xE3069283
assert crc64nvme(b"123456789") == 0xAE8B14860A799888


def value_bytes(kind: str, data: bytes) -> bytes:
    """The checksum of `data` as the bytes the header carries (big-endian for the CRCs)."""
    if kind == "crc32c":
        return crc32c(data).to_bytes(4, "big")
    if kind == "crc32":
        return zlib.crc32(data).to_bytes(4, "big")
    if kind == "crc64nvme":
        return crc64nvme(data).to_bytes(8, "big")
    return hashlib.new(kind, data).digest()


def to_array(kind: str, values) -> np.ndarray:
    """Header bytes of n checksums -> the library's layout: numbers for the CRCs ((n,) uint32 /
    uint64), the digest's bytes in memory as (n, 5) / (n, 8) words."""
    if kind in ("crc32c", "crc32"):
        return np.array([int.from_bytes(v, "big") for v in values], dtype=np.uint32)
    if kind == "crc64nvme":
        return np.array([int.from_bytes(v, "big") for v in values], dtype=np.uint64)
    return np.frombuffer(b"".join(values), dtype=np.uint32).reshape(len(values), -1)


def line_text(kind: str, value: bytes) -> str:
    return NAMES[kind] + ":" + base64.b64encode(value).decode()


def trailer_signature(key: bytes, region: str, service: str, last: bytes, kind: str, value: bytes) -> bytes:
    line = (line_text(kind, value) + "\n").encode()
    prefix = f"AWS4-HMAC-SHA256-TRAILER\n{ref.TIMESTAMP}\n{ref.DATE}/{region}/{service}/aws4_request\n"
    return ref._mac(key, (prefix + last.hex() + "\n" + hashlib.sha256(line).hexdigest()).encode())


def trailer_signatures(key: bytes, region: str, service: str, lasts, kind: str, values) -> np.ndarray:
    """(n, 8) uint32 from n last chunk signatures (32 bytes or 8 words each) and n header values."""
    raw = b"".join(trailer_signature(key, region, service,
                                     l if isinstance(l, bytes) else np.ascontiguousarray(l).tobytes(), kind, v)
                   for l, v in zip(lasts, values))
    return np.frombuffer(raw, dtype=np.uint32).reshape(-1, 8)


def expected(key: bytes, region: str, service: str, seeds, parts, chunk_bytes: int, kind: str):
    """Everything a trailer launch returns for `parts` (bytes each): the chunk signatures
    (signatures, 8), the checksums in the library's layout, the trailer signatures (n, 8)."""
    sigs = ref.signatures(key, region, service, seeds, parts, chunk_bytes)
    ends = np.cumsum([len(ref.cut(bytes(p), chunk_bytes)) + 1 for p in parts]) - 1
    values = [value_bytes(kind, bytes(p)) for p in parts]
    return sigs, to_array(kind, values), trailer_signatures(key, region, service, sigs[ends], kind, values)
