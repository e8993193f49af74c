// chunk_body_wrappers_test.cpp -- the C++ body wrappers of include/s3hash_batch.hpp (namespace
// s3h) on the AWS documentation's example, 66,560 x 'a' at 64 KiB chunks: the two known lengths
// (66,824 and 66,946 with a CRC-32C trailer), the bodies byte for byte against text put together
// here, two parts packed back to back, and the argument errors.  Needs no GPU (built by
// `make cpptests`, run by tests/test_chunk_body_cpp.py).
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

static const char* const kSig[3] = {"ad80c730a21e5b8d04586a2213dd63b9a0e99e0e2307b0ade35a65485a288648",
                                    "0055627c9e194cb4542bae2aa5492e3c1575bbb81b612b7d234b86a503ef5497",
                                    "b6c6ea8a5354eaf15b3cb7646744f4275b71ea724fed81ceb9323e279d449df9"};

int main() {
  const std::vector<uint8_t> key =
      s3h::sigv4_signing_key("wJalrXUtnFEMI/K7MDENG/bPxRfiCYEXAMPLEKEY", "20130524", "us-east-1", "s3");
  const s3h::ChunkSignContext ctx(key, "20130524T000000Z", "20130524", "us-east-1");
  const std::vector<uint8_t> data(66560, 'a');
  std::vector<uint32_t> digests(16);
  sha256::sha256(data.data(), 65536, digests.data());
  sha256::sha256(data.data() + 65536, 1024, digests.data() + 8);
  const std::vector<uint32_t> seed = unhex("4f232c4386841ef735655705268965c44a0e4690baa4adea153f7db9fa80a0a9");
  const std::vector<uint32_t> sig = ctx.signatures(digests, {2}, seed);

  // the lengths: 65,626 + 1,112 + 86, and 84 + 124 at the end with the CRC-32C trailer
  s3h::ChunkBodyGeometry g = s3h::chunk_body_geometry({66560}, 65536);
  CHECK(g.total == 66824 && g.lengths[0] == 66824 && g.offsets[0] == 0);
  CHECK(s3h::chunk_body_geometry({66560}, 65536, S3H_TRAILER_CRC32C).total == 66946);
  g = s3h::chunk_body_geometry({66560, 0, 15}, 65536, S3H_TRAILER_CRC64NVME);
  CHECK(g.lengths[0] == 66824 - 2 + 37 + 94 && g.lengths[1] == 84 + 37 + 94 && g.lengths[2] == 1 + 85 + 15 + 84 + 37 + 94);
  CHECK(g.offsets[1] == g.lengths[0] && g.offsets[2] == g.lengths[0] + g.lengths[1]);
  CHECK(g.total == g.offsets[2] + g.lengths[2]);

  // the plain body
  const std::string a64k(65536, 'a'), a1k(1024, 'a');
  const std::string plain = std::string("10000;chunk-signature=") + kSig[0] + "\r\n" + a64k + "\r\n" +
                            "400;chunk-signature=" + kSig[1] + "\r\n" + a1k + "\r\n" +
                            "0;chunk-signature=" + kSig[2] + "\r\n";
  std::vector<uint8_t> body = s3h::chunk_body_host({data.data()}, {66560}, 65536, sig);
  CHECK(body.size() == 66824);
  CHECK(std::string(body.begin(), body.end()) == plain + "\r\n");

  // the trailer form (any signatures frame alike: the assembler only renders them)
  const std::vector<uint32_t> crc = {s3h_cpu_crc(S3H_CRC32C, data.data(), data.size(), 0)};
  const std::vector<uint32_t> tsig = unhex("d81f82fc3505edab99d459891051a732e8730629a2e4a59689829ca17fe2e435");
  body = s3h::chunk_body_host({data.data()}, {66560}, 65536, sig, S3H_TRAILER_CRC32C, crc.data(), tsig);
  CHECK(body.size() == 66946);
  CHECK(std::string(body.begin(), body.end()) ==
        plain + "x-amz-checksum-crc32c:sOO8/Q==\r\n"
                "x-amz-trailer-signature:d81f82fc3505edab99d459891051a732e8730629a2e4a59689829ca17fe2e435\r\n\r\n");
  // ... and what the older text functions give sits where the rule says
  const std::string text(body.begin(), body.end());
  CHECK(text.compare(0, 5 + 83, s3h::chunk_header_text(65536, sig.data())) == 0);
  CHECK(text.compare(65626, 3 + 83, s3h::chunk_header_text(1024, sig.data() + 8)) == 0);
  CHECK(text.compare(66738 + 84, std::string::npos, s3h::chunk_trailer_text(S3H_TRAILER_CRC32C, crc.data(), tsig.data())) == 0);

  // two parts, the second empty: packed back to back
  std::vector<uint32_t> sig2(sig);
  sig2.insert(sig2.end(), sig.begin(), sig.begin() + 8);
  body = s3h::chunk_body_host({data.data(), nullptr}, {66560, 0}, 65536, sig2);
  CHECK(body.size() == 66824 + 86);
  CHECK(std::string(body.begin() + 66824, body.end()) == std::string("0;chunk-signature=") + kSig[0] + "\r\n\r\n");

  // argument errors
  CHECK(throws_einval([&] { s3h::chunk_body_geometry({100}, 0); }));
  CHECK(throws_einval([&] { s3h::chunk_body_geometry({100}, 64, 5); }));
  CHECK(throws_einval([&] { s3h::chunk_body_geometry({}, 64); }));
  CHECK(throws_einval([&] { s3h::chunk_body_host({data.data()}, {66560}, 65536, sig, S3H_TRAILER_CRC32C, nullptr, tsig); }));
  CHECK(throws_einval([&] { s3h::chunk_body_host({data.data()}, {66560}, 65536, sig, -1, crc.data()); }));
  CHECK(throws_einval([&] { s3h::chunk_body_host({nullptr}, {66560}, 65536, sig); }));
  CHECK(s3h_cpu_chunk_body(nullptr, nullptr, 1, 64, sig.data(), -1, nullptr, nullptr, body.data(), nullptr) == S3H_EINVAL);
  // the device forms do not take a digest checksum (refused before a device is looked for)
  CHECK(throws_einval([&] {
    s3h::chunk_body_batch_device(0, ctx, S3H_TRAILER_SHA256, data.data(), {0}, {100}, 64, seed);
  }));
  bool threw = false;
  try {
    s3h::chunk_body_host({data.data()}, {66560}, 65536, seed);  // one signature for three
  } catch (const std::invalid_argument&) {
    threw = true;
  }
  CHECK(threw);
  std::puts("ok");
  return 0;
}
