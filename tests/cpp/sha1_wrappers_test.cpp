// sha1_wrappers_test.cpp -- the C++ SHA-1 wrappers of include/s3hash_batch.hpp (namespace sha1)
// against known answers, and the argument errors that need no GPU (compiled and run by
// tests/test_sha1_cpu.py).  With the argument "gpu" and a file path (tests/test_gpu_sha1_host.py)
// it also runs the host-resident forms on a device: the file holds the bytes 0, 1, ..., 255
// repeated, and every digest is compared with the CPU function's.
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

static std::string hex(const std::vector<uint32_t>& d) {
  std::string s;
  char b[3];
  const uint8_t* p = reinterpret_cast<const uint8_t*>(d.data());
  for (size_t i = 0; i < 4 * d.size(); ++i) {
    std::snprintf(b, sizeof b, "%02x", p[i]);
    s += b;
  }
  return s;
}

static int gpu_part(const char* path) {
  // 40 parts of one buffer: lengths around the block boundaries and a few long ones
  std::vector<uint8_t> buf(3 << 20);
  for (size_t i = 0; i < buf.size(); ++i) buf[i] = uint8_t(i);
  std::vector<const uint8_t*> parts;
  std::vector<uint64_t> offs, lens;
  uint64_t at = 0;
  for (uint64_t L : {0, 1, 55, 56, 63, 64, 65, 119, 120, 128, 1000, 4096, 70001, 262144, 600007}) {
    for (int rep = 0; rep < 2; ++rep) {
      offs.push_back(at);
      lens.push_back(L);
      parts.push_back(buf.data() + at);
      at += L + 3;
    }
  }
  CHECK(at <= buf.size());
  std::vector<uint32_t> want;
  for (size_t i = 0; i < parts.size(); ++i) {
    const std::vector<uint32_t> h = sha1::sha1(parts[i], lens[i]);
    want.insert(want.end(), h.begin(), h.end());
  }
  CHECK(sha1::sha1_batch(parts, lens) == want);
  CHECK(sha1::sha1_batch(parts, lens, 1, 4096) == want);
  const sha1::Sha256Sha1 both = sha1::sha256_sha1_batch(parts, lens);
  CHECK(both.sha1 == want);
  CHECK(both.sha256 == sha256::sha256_batch(parts, lens));
  CHECK(sha1::file_part_sha1(path, offs, lens) == want);
  const sha1::Sha256Sha1 fboth = sha1::file_part_sha256_sha1(path, offs, lens);
  CHECK(fboth.sha1 == want && fboth.sha256 == both.sha256);
  // a range past the end of the file
  CHECK(throws_einval([&] { sha1::file_part_sha1(path, {buf.size() - 1}, {2}); }));
  CHECK(throws_einval([&] { sha1::file_part_sha256_sha1(path, {buf.size() - 1}, {2}); }));
  return 0;
}

int main(int argc, char** argv) {
  const uint8_t* abc = reinterpret_cast<const uint8_t*>("abc");
  const std::vector<uint32_t> h = sha1::sha1(abc, 3);
  CHECK(hex(h) == "a9993e364706816aba3e25717850c26c9cd0d89d");
  CHECK(hex(sha1::sha1(abc, 0)) == "da39a3ee5e6b4b0d3255bfef95601890afd80709");
  CHECK(hex(sha1::sha1(nullptr, 0)) == "da39a3ee5e6b4b0d3255bfef95601890afd80709");
  CHECK(sha1::checksum_text(h) == "qZk+NkcGgWq6PiVxeFDCbJzQ2J0=");
  // composite of one part: SHA-1 of the 20 digest bytes, then "-1"
  const std::vector<uint32_t> hh = sha1::sha1(reinterpret_cast<const uint8_t*>(h.data()), 20);
  CHECK(sha1::composite_checksum_text(h) == sha1::checksum_text(hh) + "-1");
  std::vector<uint32_t> two(h);
  two.insert(two.end(), hh.begin(), hh.end());
  const std::string c2 = sha1::composite_checksum_text(two);
  CHECK(c2.size() == 30 && c2.substr(28) == "-2");
  // SHA-256 digests through the same helper
  std::vector<uint32_t> s(8);
  s3h_cpu_sha256(abc, 3, s.data());
  CHECK(sha1::checksum_text(s, S3H_ALGO_SHA256) == "ungWv48Bz+pBQUDeXa4iI7ADYaOWF3qctBD/YfIAFa0=");
  CHECK(sha1::composite_checksum_text(s, S3H_ALGO_SHA256).size() == 46);

  bool bad = false;
  try {
    sha1::checksum_text(two);
  } catch (const std::invalid_argument&) {
    bad = true;
  }
  CHECK(bad);
  char out[S3H_DIGEST_CHECKSUM_MAX];
  CHECK(s3h_digest_checksum_text(S3H_ALGO_MD5, h.data(), 1, 0, out, sizeof out) == S3H_EINVAL);
  CHECK(s3h_digest_checksum_text(S3H_ALGO_SHA1, h.data(), 2, 0, out, sizeof out) == S3H_EINVAL);
  CHECK(s3h_digest_checksum_text(S3H_ALGO_SHA1, h.data(), 1, 0, out, sizeof out - 1) == S3H_EINVAL);
  CHECK(s3h_digest_checksum_text(S3H_ALGO_SHA1, nullptr, 1, 0, out, sizeof out) == S3H_EINVAL);

  // plans: reported before any device is looked for
  const uint64_t zero[1] = {0};
  s3h_plan_t plan = nullptr;
  CHECK(s3h_plan_create_ex(0, 3, zero, zero, 1, S3H_KERNEL_AUTO, &plan) == S3H_EINVAL);
  CHECK(s3h_plan_create_ex(0, S3H_ALGO_SHA1, zero, zero, 1, S3H_KERNEL_SKEW, &plan) == S3H_EINVAL);
  CHECK(std::strstr(s3h_last_error(), "SHA-1"));
  CHECK(plan == nullptr);
  // digest pointers: SHA-1 takes any 4-byte aligned one, SHA-256 needs 16; a pointer that misses
  // it is refused before any device is looked for (the pointers are never dereferenced)
  alignas(16) static uint8_t fake[64];
  CHECK(throws_einval([&] { sha1::sha1_batch_device(0, fake, {0}, {3}, reinterpret_cast<uint32_t*>(fake + 18)); }));
  CHECK(std::strstr(s3h_last_error(), "4-byte aligned"));
  CHECK(throws_einval([&] { sha256::sha256_batch_device(0, fake, {0}, {3}, reinterpret_cast<uint32_t*>(fake + 20)); }));
  CHECK(std::strstr(s3h_last_error(), "16-byte aligned"));

  // empty batches are no call at all; size mismatches never reach the library
  CHECK(sha1::sha1_batch({}, {}).empty());
  const sha1::Sha256Sha1 none = sha1::sha256_sha1_batch({}, {});
  CHECK(none.sha256.empty() && none.sha1.empty());
  CHECK(sha1::file_part_sha1("/dev/null", {}, {}).empty());
  CHECK(sha1::file_part_sha256_sha1("/dev/null", {}, {}).sha1.empty());
  const uint8_t byte = 'a';
  bad = false;
  try {
    sha1::sha1_batch({&byte}, {1, 2});
  } catch (const std::invalid_argument&) {
    bad = true;
  }
  CHECK(bad);

  if (argc > 2 && std::strcmp(argv[1], "gpu") == 0)
    if (int rc = gpu_part(argv[2])) return rc;
  std::puts("ok");
  return 0;
}
