"""SigV4 chunk signatures (STREAMING-AWS4-HMAC-SHA256-PAYLOAD) from hashlib + hmac alone, straight
from the definition: the reference of the chunk-signing tests, independent of the library.

    string = "AWS4-HMAC-SHA256-PAYLOAD\\n" timestamp "\\n" date/region/service/aws4_request "\\n"
             hex(previous signature) "\\n" hex(sha256("")) "\\n" hex(sha256(chunk))
    signature = HMAC-SHA256(signing_key, string)
"""
import hashlib
import hmac

import numpy as np

SECRET = "wJalrXUtnFEMI/K7MDENG/bPxRfiCYEXAMPLEKEY"
DATE, TIMESTAMP = "20130524", "20130524T000000Z"
# the AWS documentation's example: 66,560 x 'a' at chunk size 65,536 (us-east-1, s3)
KNOWN_KEY = "dbb893acc010964918f1fd433add87c70e8b0db6be30c1fbeafefa5ec6ba8378"
KNOWN_SEED = "4f232c4386841ef735655705268965c44a0e4690baa4adea153f7db9fa80a0a9"
KNOWN_SIGNATURES = ("ad80c730a21e5b8d04586a2213dd63b9a0e99e0e2307b0ade35a65485a288648",
                    "0055627c9e194cb4542bae2aa5492e3c1575bbb81b612b7d234b86a503ef5497",
                    "b6c6ea8a5354eaf15b3cb7646744f4275b71ea724fed81ceb9323e279d449df9")
EMPTY = hashlib.sha256(b"").hexdigest()
# remainders r = |prefix| mod 64 the tests cover: the known answer's 13; 53 / 54, where the inner
# tail goes from 4 to 5 blocks; every byte alignment on both sides of it and of the block end;
# 38 with a prefix of 166 bytes (two whole prefix blocks; so has r = 0, at 128 bytes)
REMAINDERS = (13, 51, 52, 53, 54, 55, 62, 63, 0, 1, 38)


def _mac(key: bytes, msg: bytes) -> bytes:
    return hmac.new(key, msg, hashlib.sha256).digest()


def signing_key(secret: str, date: str, region: str, service: str) -> bytes:
    k = _mac(("AWS4" + secret).encode(), date.encode())
    return _mac(_mac(_mac(k, region.encode()), service.encode()), b"aws4_request")


def names_for(r: int) -> tuple[str, str]:
    """A region and a service whose prefix, 66 + |region| + |service| bytes, leaves remainder r
    (r = 38: 166 bytes)."""
    total = 100 if r == 38 else (r - 2) % 64
    if total == 11:
        return "us-east-1", "s3"
    return "r" * (total - 2), "s3"


def chain(key: bytes, region: str, service: str, seed: bytes, chunk_digests) -> list[bytes]:
    """Signatures of one part: its data chunks' digests (32 bytes each), then the final chunk."""
    prefix = f"AWS4-HMAC-SHA256-PAYLOAD\n{TIMESTAMP}\n{DATE}/{region}/{service}/aws4_request\n"
    assert len(prefix) == 66 + len(region) + len(service)
    prev, out = seed, []
    for d in list(chunk_digests) + [hashlib.sha256(b"").digest()]:
        prev = _mac(key, (prefix + prev.hex() + "\n" + EMPTY + "\n" + bytes(d).hex()).encode())
        out.append(prev)
    return out


def cut(part: bytes, chunk_bytes: int) -> list[bytes]:
    return [part[i:i + chunk_bytes] for i in range(0, len(part), chunk_bytes)]


def signatures(key: bytes, region: str, service: str, seeds, parts, chunk_bytes: int) -> np.ndarray:
    """(signatures, 8) uint32, part-major, of `parts` (bytes each) from the (n, 8)-word seeds."""
    seeds = np.ascontiguousarray(seeds, dtype=np.uint32).reshape(-1, 8)
    raw = b""
    for seed, part in zip(seeds, parts):
        digs = [hashlib.sha256(c).digest() for c in cut(bytes(part), chunk_bytes)]
        raw += b"".join(chain(key, region, service, seed.tobytes(), digs))
    return np.frombuffer(raw, dtype=np.uint32).reshape(-1, 8)
