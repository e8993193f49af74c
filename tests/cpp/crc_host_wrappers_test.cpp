// crc_host_wrappers_test.cpp -- the host-resident CRC entry points (s3h_crc_batch_host,
// s3h_sha256_crc_batch_host, s3h_sha256_crc_file_parts) and their C++ wrappers in
// include/s3hash_batch.hpp, namespace crc: the argument errors that need no GPU (compiled and
// run by tests/test_crc_range_cpu.py; tests/test_gpu_crc_host.py runs it again with a device).
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

int main(int argc, char** argv) {
  const uint8_t byte = 'a';
  const uint8_t* part[1] = {&byte};
  const uint64_t len[1] = {1}, off[1] = {0};
  uint32_t sha[8], crcs[1];
  const char* path = argc > 1 ? argv[1] : "/dev/null";
  for (int bad : {2, -1, 7, 0x100}) {  // an unknown checksum, whatever else is passed
    CHECK(s3h_crc_batch_host(bad, part, len, 1, crcs, 0, 0) == S3H_EINVAL);
    CHECK(s3h_sha256_crc_batch_host(bad, part, len, 1, sha, crcs, 0, 0) == S3H_EINVAL);
    CHECK(s3h_sha256_crc_file_parts(bad, path, off, len, 1, sha, crcs, 0, 0) == S3H_EINVAL);
    CHECK(std::strstr(s3h_last_error(), "unknown checksum"));
  }
  for (int crc : {S3H_CRC32C, S3H_CRC32}) {  // null pointers
    CHECK(s3h_crc_batch_host(crc, nullptr, len, 1, crcs, 0, 0) == S3H_EINVAL);
    CHECK(s3h_crc_batch_host(crc, part, nullptr, 1, crcs, 0, 0) == S3H_EINVAL);
    CHECK(s3h_crc_batch_host(crc, part, len, 1, nullptr, 0, 0) == S3H_EINVAL);
    CHECK(s3h_sha256_crc_batch_host(crc, nullptr, len, 1, sha, crcs, 0, 0) == S3H_EINVAL);
    CHECK(s3h_sha256_crc_batch_host(crc, part, nullptr, 1, sha, crcs, 0, 0) == S3H_EINVAL);
    CHECK(s3h_sha256_crc_batch_host(crc, part, len, 1, nullptr, crcs, 0, 0) == S3H_EINVAL);
    CHECK(s3h_sha256_crc_batch_host(crc, part, len, 1, sha, nullptr, 0, 0) == S3H_EINVAL);
    CHECK(s3h_sha256_crc_file_parts(crc, nullptr, off, len, 1, sha, crcs, 0, 0) == S3H_EINVAL);
    CHECK(s3h_sha256_crc_file_parts(crc, path, nullptr, len, 1, sha, crcs, 0, 0) == S3H_EINVAL);
    CHECK(s3h_sha256_crc_file_parts(crc, path, off, nullptr, 1, sha, crcs, 0, 0) == S3H_EINVAL);
    CHECK(s3h_sha256_crc_file_parts(crc, path, off, len, 1, nullptr, crcs, 0, 0) == S3H_EINVAL);
    CHECK(s3h_sha256_crc_file_parts(crc, path, off, len, 1, sha, nullptr, 0, 0) == S3H_EINVAL);
  }
  // the wrappers: errors arrive as batch_error, empty batches are no call at all
  const std::vector<const uint8_t*> parts{&byte};
  const std::vector<uint64_t> lens{1}, offs{0};
  CHECK(throws_einval([&] { crc::crc_batch(2, parts, lens); }));
  CHECK(throws_einval([&] { crc::sha256_crc_batch(2, parts, lens); }));
  CHECK(throws_einval([&] { crc::file_part_sha256_crc(2, path, offs, lens); }));
  CHECK(crc::crc_batch(S3H_CRC32, {}, {}).empty());
  const crc::Sha256Crc none = crc::sha256_crc_batch(S3H_CRC32C, {}, {});
  CHECK(none.sha256.empty() && none.crc.empty());
  CHECK(crc::file_part_sha256_crc(S3H_CRC32C, path, {}, {}).crc.empty());
  std::puts("ok");
  return 0;
}
