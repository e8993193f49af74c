// crc64_wrappers_test.cpp -- the C++ CRC-64/NVME wrappers of include/s3hash_batch.hpp
// (namespace crc64) against known answers, and the argument errors of the host-resident entry
// points that need no GPU (compiled and run by tests/test_crc64_cpu.py).
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

int main() {
  const uint8_t* m = reinterpret_cast<const uint8_t*>("123456789");
  const uint64_t check = 0xAE8B14860A799888ull;
  CHECK(crc64::crc(m, 9) == check);
  CHECK(crc64::crc(m, 0) == 0);
  CHECK(crc64::crc(m + 4, 5, crc64::crc(m, 4)) == check);
  const uint64_t a = crc64::crc(m, 4), b = crc64::crc(m + 4, 5);
  CHECK(crc64::combine(a, b, 5) == check);
  CHECK(crc64::object_crc({a, 0, b}, {4, 0, 5}) == check);
  CHECK(crc64::checksum_text(check) == "rosUhgp5mIg=");
  CHECK(crc64::checksum_text(0) == "AAAAAAAAAAA=");
  CHECK(throws_einval([&] { crc64::object_crc({}, {}); }));

  // host-resident forms: null pointers and empty batches, before any device is looked for
  const uint8_t byte = 'a';
  const uint8_t* part[1] = {&byte};
  const uint64_t len[1] = {1}, off[1] = {0};
  uint32_t sha[8];
  uint64_t crcs[1];
  const char* path = "/dev/null";
  CHECK(s3h_crc64nvme_batch_host(nullptr, len, 1, crcs, 0, 0) == S3H_EINVAL);
  CHECK(s3h_crc64nvme_batch_host(part, nullptr, 1, crcs, 0, 0) == S3H_EINVAL);
  CHECK(s3h_crc64nvme_batch_host(part, len, 1, nullptr, 0, 0) == S3H_EINVAL);
  CHECK(s3h_crc64nvme_batch_host(part, len, 0, crcs, 0, 0) == S3H_EINVAL);
  CHECK(s3h_sha256_crc64nvme_batch_host(nullptr, len, 1, sha, crcs, 0, 0) == S3H_EINVAL);
  CHECK(s3h_sha256_crc64nvme_batch_host(part, nullptr, 1, sha, crcs, 0, 0) == S3H_EINVAL);
  CHECK(s3h_sha256_crc64nvme_batch_host(part, len, 1, nullptr, crcs, 0, 0) == S3H_EINVAL);
  CHECK(s3h_sha256_crc64nvme_batch_host(part, len, 1, sha, nullptr, 0, 0) == S3H_EINVAL);
  CHECK(s3h_sha256_crc64nvme_batch_host(part, len, 0, sha, crcs, 0, 0) == S3H_EINVAL);
  CHECK(s3h_sha256_crc64nvme_file_parts(nullptr, off, len, 1, sha, crcs, 0, 0) == S3H_EINVAL);
  CHECK(s3h_sha256_crc64nvme_file_parts(path, nullptr, len, 1, sha, crcs, 0, 0) == S3H_EINVAL);
  CHECK(s3h_sha256_crc64nvme_file_parts(path, off, nullptr, 1, sha, crcs, 0, 0) == S3H_EINVAL);
  CHECK(s3h_sha256_crc64nvme_file_parts(path, off, len, 1, nullptr, crcs, 0, 0) == S3H_EINVAL);
  CHECK(s3h_sha256_crc64nvme_file_parts(path, off, len, 1, sha, nullptr, 0, 0) == S3H_EINVAL);
  CHECK(crc64::crc_batch({}, {}).empty());
  const crc64::Sha256Crc64 none = crc64::sha256_crc_batch({}, {});
  CHECK(none.sha256.empty() && none.crc.empty());
  CHECK(crc64::file_part_sha256_crc(path, {}, {}).crc.empty());
  bool mismatch = false;
  try {
    crc64::crc_batch({&byte}, {1, 2});
  } catch (const std::invalid_argument&) {
    mismatch = true;
  }
  CHECK(mismatch);
  // 64-bit values are 8-byte aligned: a pointer 4 bytes off is refused before any device is
  // looked for, through the wrappers' error path (the pointers are never dereferenced)
  alignas(16) static uint8_t fake[32];
  CHECK(throws_einval([&] { crc64::crc_batch_device(0, fake, {0}, {9}, reinterpret_cast<uint64_t*>(fake + 20)); }));
  CHECK(std::strstr(s3h_last_error(), "8-byte aligned"));
  std::puts("ok");
  return 0;
}
