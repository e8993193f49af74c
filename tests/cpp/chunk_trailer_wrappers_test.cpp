// chunk_trailer_wrappers_test.cpp -- the C++ trailer-signature wrappers of include/s3hash_batch.hpp
// (namespace s3h) against the known answer in the AWS documentation's setting: 66,560 x 'a' at
// 64 KiB chunks with a CRC-32C trailer -- the chunk signatures, the header line, the trailer
// signature through the CPU link, the framing text, and the argument errors.  Needs no GPU
// (built by `make cpptests`, run by tests/test_chunk_trailer_cpp.py).
#include <cstdio>
#include <cstring>

#include "s3hash_batch.hpp"

#define CHECK(x)                                         \
  do {                                                   \
    if (!(x)) {                                          \
      std::fprintf(stderr, "failed: %s\n", #x);          \
      return 1;                                          \
    }                                                    \
  } while (0)

template <class F>
static bool throws_einval(F f) {
  try {
    f();
  } catch (const sha256::batch_error& e) {
    return e.code == S3H_EINVAL;
  }
  return false;
}

static std::string hex(const void* p, size_t n) {
  std::string s;
  char b[3];
  for (size_t i = 0; i < n; ++i) {
    std::snprintf(b, sizeof b, "%02x", static_cast<const uint8_t*>(p)[i]);
    s += b;
  }
  return s;
}

static std::vector<uint32_t> unhex(const char* text) {
  std::vector<uint32_t> w(std::strlen(text) / 8);
  uint8_t* p = reinterpret_cast<uint8_t*>(w.data());
  for (size_t i = 0; i < 4 * w.size(); ++i) {
    unsigned v = 0;
    std::sscanf(text + 2 * i, "%2x", &v);
    p[i] = uint8_t(v);
  }
  return w;
}

int main() {
  const std::vector<uint8_t> key =
      s3h::sigv4_signing_key("wJalrXUtnFEMI/K7MDENG/bPxRfiCYEXAMPLEKEY", "20130524", "us-east-1", "s3");
  const s3h::ChunkSignContext ctx(key, "20130524T000000Z", "20130524", "us-east-1");
  const std::vector<uint8_t> body(66560, 'a');
  std::vector<uint32_t> digests(16);
  sha256::sha256(body.data(), 65536, digests.data());
  sha256::sha256(body.data() + 65536, 1024, digests.data() + 8);
  const std::vector<uint32_t> seed =
      unhex("106e2a8a18243abcf37539882f36619c00e2dfc72633413f02d3b74544bfeb8e");
  const std::vector<uint32_t> sig = ctx.signatures(digests, {2}, seed);
  CHECK(hex(sig.data(), 32) == "b474d8862b1487a5145d686f57f013e54db672cee1c953b3010fb58501ef5aa2");
  CHECK(hex(sig.data() + 8, 32) == "1c1344b170168f8e65b41376b44b20fe354e373826ccbbe2c1d40a8cae51e5c7");
  CHECK(hex(sig.data() + 16, 32) == "2ca2aba2005185cf7159c6277faf83795951dd77a3a99e6e65d5c9f85863f992");

  const std::vector<uint32_t> crc = {s3h_cpu_crc(S3H_CRC32C, body.data(), body.size(), 0)};
  CHECK(s3h::trailer_line_text(S3H_TRAILER_CRC32C, crc.data()) == "x-amz-checksum-crc32c:sOO8/Q==");
  const std::vector<uint32_t> last(sig.begin() + 16, sig.end());
  const std::vector<uint32_t> tsig = s3h::trailer_signatures(ctx, S3H_TRAILER_CRC32C, crc, last);
  CHECK(tsig.size() == 8);
  CHECK(hex(tsig.data(), 32) == "d81f82fc3505edab99d459891051a732e8730629a2e4a59689829ca17fe2e435");
  CHECK(s3h::chunk_trailer_text(S3H_TRAILER_CRC32C, crc.data(), tsig.data()) ==
        "x-amz-checksum-crc32c:sOO8/Q==\r\n"
        "x-amz-trailer-signature:d81f82fc3505edab99d459891051a732e8730629a2e4a59689829ca17fe2e435\r\n\r\n");

  // two parts sign apart; a 64-bit value and a digest have lines of their own
  std::vector<uint32_t> last2(last);
  last2.insert(last2.end(), sig.begin(), sig.begin() + 8);
  const std::vector<uint32_t> two = s3h::trailer_signatures(ctx, S3H_TRAILER_CRC32C, std::vector<uint32_t>{crc[0], 0}, last2);
  CHECK(two.size() == 16 && std::equal(tsig.begin(), tsig.end(), two.begin()));
  CHECK(!std::equal(tsig.begin(), tsig.end(), two.begin() + 8));
  const std::vector<uint64_t> zero64 = {0};
  CHECK(s3h::trailer_line_text(S3H_TRAILER_CRC64NVME, zero64.data()) == "x-amz-checksum-crc64nvme:AAAAAAAAAAA=");
  CHECK(s3h::trailer_signatures(ctx, S3H_TRAILER_CRC64NVME, zero64, last).size() == 8);
  std::vector<uint32_t> sha(8);
  sha256::sha256(body.data(), 0, sha.data());
  CHECK(s3h::trailer_line_text(S3H_TRAILER_SHA256, sha.data()) ==
        "x-amz-checksum-sha256:47DEQpj8HBSa+/TImW+5JCeuQeRkm5NMpJWZG3hSuFU=");
  CHECK(s3h::trailer_signatures(ctx, S3H_TRAILER_SHA256, sha, last).size() == 8);

  // argument errors
  CHECK(throws_einval([&] { s3h::trailer_line_text(5, crc.data()); }));
  CHECK(throws_einval([&] { s3h::trailer_line_text(S3H_TRAILER_CRC32, nullptr); }));
  CHECK(throws_einval([&] { s3h::chunk_trailer_text(S3H_TRAILER_CRC32, crc.data(), nullptr); }));
  CHECK(throws_einval([&] { s3h::trailer_signatures(ctx, 7, crc, last); }));
  // the device forms do not take a digest checksum (refused before a device is looked for)
  CHECK(throws_einval([&] { s3h::ChunkTrailerPlan bad(0, S3H_TRAILER_SHA1, {0}, {100}, 64); }));
  CHECK(throws_einval([&] { s3h::ChunkTrailerPlan bad(0, S3H_TRAILER_CRC32C, {0}, {100}, 0); }));
  CHECK(throws_einval([&] {
    s3h::chunk_trailer_signatures_host(ctx, S3H_TRAILER_CRC32C, {body.data()}, {66560}, 0, seed);
  }));
  bool threw = false;
  try {
    s3h::trailer_signatures(ctx, S3H_TRAILER_CRC64NVME, crc, last);  // 32-bit values for a 64-bit kind
  } catch (const std::invalid_argument&) {
    threw = true;
  }
  CHECK(threw);
  std::puts("ok");
  return 0;
}
