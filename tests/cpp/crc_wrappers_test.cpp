// crc_wrappers_test.cpp -- the C++ CRC wrappers of include/s3hash_batch.hpp against known
// answers, on the CPU (compiled and run by tests/test_crc_cpu.py).
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

int main() {
  const uint8_t* m = reinterpret_cast<const uint8_t*>("123456789");
  CHECK(crc::crc(S3H_CRC32C, m, 9) == 0xE3069283u);
  CHECK(crc::crc(S3H_CRC32, m, 9) == 0xCBF43926u);
  CHECK(crc::crc(S3H_CRC32C, m + 4, 5, crc::crc(S3H_CRC32C, m, 4)) == 0xE3069283u);
  const uint32_t a = crc::crc(S3H_CRC32, m, 4), b = crc::crc(S3H_CRC32, m + 4, 5);
  CHECK(crc::combine(S3H_CRC32, a, b, 5) == 0xCBF43926u);
  CHECK(crc::object_crc(S3H_CRC32, {a, 0, b}, {4, 0, 5}) == 0xCBF43926u);
  CHECK(crc::checksum_text(S3H_CRC32C, 0xE3069283u) == "4waSgw==");
  const std::string comp = crc::composite_checksum_text(S3H_CRC32C, {a, b});
  CHECK(comp.size() == 10 && comp.substr(8) == "-2");
  bool threw = false;
  try {
    crc::combine(7, a, b, 5);
  } catch (const sha256::batch_error& e) {
    threw = e.code == S3H_EINVAL;
  }
  CHECK(threw);
  // a CRC pointer that is not 4-byte aligned is refused before any device is looked for, and
  // reported through the wrappers' error path (the pointers are never dereferenced)
  alignas(16) static uint8_t fake[32];
  threw = false;
  try {
    crc::crc_batch_device(0, S3H_CRC32C, fake, {0}, {9}, reinterpret_cast<uint32_t*>(fake + 18));
  } catch (const sha256::batch_error& e) {
    threw = e.code == S3H_EINVAL && std::strstr(e.what(), "aligned");
  }
  CHECK(threw);
  std::puts("ok");
  return 0;
}
