// chunk_sign_wrappers_test.cpp -- the C++ chunk-signing wrappers of include/s3hash_batch.hpp
// (namespace s3h) against the AWS documentation's example: signing key, the three chunk
// signatures of 66,560 x 'a' at 64 KiB chunks through the CPU chain, the framing line, and the
// argument errors.  Needs no GPU (built by `make cpptests`, run by tests/test_chunk_sign_cpp.py).
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

static std::string hex(const uint8_t* p, size_t n) {
  std::string s;
  char b[3];
  for (size_t i = 0; i < n; ++i) {
    std::snprintf(b, sizeof b, "%02x", p[i]);
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
  CHECK(hex(key.data(), 32) == "dbb893acc010964918f1fd433add87c70e8b0db6be30c1fbeafefa5ec6ba8378");

  const s3h::ChunkSignContext ctx(key, "20130524T000000Z", "20130524", "us-east-1");
  const std::vector<uint8_t> body(66560, 'a');
  std::vector<uint32_t> digests(16);
  sha256::sha256(body.data(), 65536, digests.data());
  sha256::sha256(body.data() + 65536, 1024, digests.data() + 8);
  const std::vector<uint32_t> seed =
      unhex("4f232c4386841ef735655705268965c44a0e4690baa4adea153f7db9fa80a0a9");
  const std::vector<uint32_t> sig = ctx.signatures(digests, {2}, seed);
  CHECK(sig.size() == 24);
  const uint8_t* raw = reinterpret_cast<const uint8_t*>(sig.data());
  CHECK(hex(raw, 32) == "ad80c730a21e5b8d04586a2213dd63b9a0e99e0e2307b0ade35a65485a288648");
  CHECK(hex(raw + 32, 32) == "0055627c9e194cb4542bae2aa5492e3c1575bbb81b612b7d234b86a503ef5497");
  CHECK(hex(raw + 64, 32) == "b6c6ea8a5354eaf15b3cb7646744f4275b71ea724fed81ceb9323e279d449df9");
  CHECK(s3h::chunk_header_text(65536, sig.data()) ==
        "10000;chunk-signature=ad80c730a21e5b8d04586a2213dd63b9a0e99e0e2307b0ade35a65485a288648\r\n");
  CHECK(s3h::chunk_header_text(0, sig.data() + 16) ==
        "0;chunk-signature=b6c6ea8a5354eaf15b3cb7646744f4275b71ea724fed81ceb9323e279d449df9\r\n");

  // an empty part has its final chunk's signature alone; two parts chain apart
  std::vector<uint32_t> seeds2(seed);
  seeds2.insert(seeds2.end(), seed.begin(), seed.end());
  const std::vector<uint32_t> two = ctx.signatures(digests, {2, 0}, seeds2);
  CHECK(two.size() == 32 && std::equal(sig.begin(), sig.end(), two.begin()));
  const std::vector<uint32_t> lone = ctx.signatures({}, {0}, seed);
  CHECK(lone.size() == 8 && std::equal(lone.begin(), lone.end(), two.begin() + 24));

  // argument errors
  CHECK(throws_einval([&] { s3h::ChunkSignContext bad(key, "20130524T000000", "20130524", "us-east-1"); }));
  CHECK(throws_einval([&] { s3h::ChunkSignContext bad(key, "20130524T000000Z", "2013052", "us-east-1"); }));
  CHECK(throws_einval([&] { s3h::ChunkSignContext bad(key, "20130524T000000Z", "20130524", ""); }));
  CHECK(throws_einval([&] { s3h::ChunkSignContext bad(key, "20130524T000000Z", "20130524", std::string(189, 'r')); }));
  CHECK(throws_einval([&] { s3h::chunk_signatures_host(ctx, {body.data()}, {66560}, 0, seed); }));
  bool threw = false;
  try {
    ctx.signatures(digests, {3}, seed);
  } catch (const std::invalid_argument&) {
    threw = true;
  }
  CHECK(threw);
  std::puts("ok");
  return 0;
}
