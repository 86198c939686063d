// Stand-alone host program for the argument-checking paths of csrc/boundary.hip (the launchers return before any HIP call): built
// with the host sanitizers and run on its own, never loaded into Python.
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined tools/boundary_argcheck.cpp \
//         ape_amd/csrc/boundary.hip ape_amd/csrc/error.cpp ape_amd/csrc/meter.cpp -o /tmp/boundary_argcheck && /tmp/boundary_argcheck
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../include/ape_hip.h"

static int failures = 0;

static void expect(bool refused_or_ok, const char* what, const char* needle) {
  const char* msg = ape_hip_last_error();
  if (!refused_or_ok || (needle && (!msg || !strstr(msg, needle)))) {
    printf("FAIL %s (message: %s)\n", what, msg ? msg : "(none)");
    ++failures;
  }
}

int main() {
  uint8_t* one = (uint8_t*)(uintptr_t)64;                         // never dereferenced
  uint64_t* w1 = (uint64_t*)(uintptr_t)64;
  uint64_t* w2 = (uint64_t*)(uintptr_t)4096;
  int64_t* a1 = (int64_t*)(uintptr_t)64;

  expect(ape_hip_mask_pack_rows(nullptr, 1, 4, 65, w1, 8, a1, nullptr) != 0, "pack_rows: null masks", "null");
  expect(ape_hip_mask_pack_rows(one, 1, 4, 65, nullptr, 8, a1, nullptr) != 0, "pack_rows: null bits", "null");
  expect(ape_hip_mask_pack_rows(one, 1, 4, 65, w1, 8, nullptr, nullptr) != 0, "pack_rows: null area", "null");
  expect(ape_hip_mask_pack_rows(one, -1, 4, 65, w1, 8, a1, nullptr) != 0, "pack_rows: negative n", "negative");
  expect(ape_hip_mask_pack_rows(one, 1, 0, 65, w1, 8, a1, nullptr) != 0, "pack_rows: H = 0", "at least 1");
  expect(ape_hip_mask_pack_rows(one, 1, 4, 0, w1, 8, a1, nullptr) != 0, "pack_rows: W = 0", "at least 1");
  expect(ape_hip_mask_pack_rows(one, 1, 4, 65, w1, 7, a1, nullptr) != 0, "pack_rows: short ldb", "ldb");
  expect(ape_hip_mask_pack_rows(one, 1, 1 << 30, 1 << 30, w1, (size_t)1 << 40, a1, nullptr) != 0, "pack_rows: too large", "too large");
  expect(ape_hip_mask_pack_rows(one, 1, 2147483647, 2147483647, w1, (size_t)1 << 60, a1, nullptr) != 0, "pack_rows: INT_MAX", "too large");
  expect(ape_hip_mask_pack_rows(nullptr, 0, 4, 65, nullptr, 8, nullptr, nullptr) == 0, "pack_rows: n = 0", nullptr);

  expect(ape_hip_bitmask_boundary(w1, 1, 4, 65, 0, 8, w2, 8, a1, nullptr) != 0, "boundary: d = 0", "d = 0");
  expect(ape_hip_bitmask_boundary(w1, 1, 4, 65, -2147483647 - 1, 8, w2, 8, a1, nullptr) != 0, "boundary: d = INT_MIN", "d = -");
  expect(ape_hip_bitmask_boundary(w1, 1, 0, 65, 1, 8, w2, 8, a1, nullptr) != 0, "boundary: H = 0", "at least 1");
  expect(ape_hip_bitmask_boundary(nullptr, 1, 4, 65, 1, 8, w2, 8, a1, nullptr) != 0, "boundary: null bits", "null");
  expect(ape_hip_bitmask_boundary(w1, 1, 4, 65, 1, 8, nullptr, 8, a1, nullptr) != 0, "boundary: null bbits", "null");
  expect(ape_hip_bitmask_boundary(w1, 1, 4, 65, 1, 8, w2, 8, nullptr, nullptr) != 0, "boundary: null barea", "null");
  expect(ape_hip_bitmask_boundary(w1, 1, 4, 65, 1, 7, w2, 8, a1, nullptr) != 0, "boundary: short ldb", "ldb");
  expect(ape_hip_bitmask_boundary(w1, 1, 4, 65, 1, 8, w2, 7, a1, nullptr) != 0, "boundary: short ldo", "ldo");
  expect(ape_hip_bitmask_boundary(w1, 1, 4, 65, 1, 8, w1, 8, a1, nullptr) != 0, "boundary: in place", "in place");
  expect(ape_hip_bitmask_boundary(w1, 1, 2147483647, 2147483647, 2147483647, (size_t)1 << 60, w2, (size_t)1 << 60, a1, nullptr) != 0,
         "boundary: INT_MAX", "too large");
  expect(ape_hip_bitmask_boundary(nullptr, 0, 4, 65, 1, 8, nullptr, 8, nullptr, nullptr) == 0, "boundary: n = 0", nullptr);

  int rows = -1, words = -1;
  expect(ape_hip_bitmask_boundary_tile(1024, 1024, 29, 65536, &rows, &words) == (116 + 58) * 16 * 16 && rows == 116 && words == 16,
         "tile: 1024^2, d = 29", nullptr);
  expect(ape_hip_bitmask_boundary_tile(2147483647, 2147483647, 1073741823, 65536, &rows, &words) < 0, "tile: INT_MAX", nullptr);
  expect(ape_hip_bitmask_boundary_tile(70, 200, 63, 65536, &rows, &words) == 0 && rows == 0 && words == 0, "tile: band is the mask", nullptr);
  expect(ape_hip_bitmask_boundary_tile(4, 4, 1, 65536, nullptr, &words) != 0, "tile: null", "null");

  expect(ape_hip_bitmask_unpack_rows(nullptr, 1, 4, 65, 8, one, nullptr) != 0, "unpack_rows: null bits", "null");
  expect(ape_hip_bitmask_unpack_rows(w1, 1, 4, 65, 8, nullptr, nullptr) != 0, "unpack_rows: null masks", "null");
  expect(ape_hip_bitmask_unpack_rows(w1, 1, 4, 0, 8, one, nullptr) != 0, "unpack_rows: W = 0", "at least 1");
  expect(ape_hip_bitmask_unpack_rows(w1, 1, 4, 65, 7, one, nullptr) != 0, "unpack_rows: short ldb", "ldb");
  expect(ape_hip_bitmask_unpack_rows(w1, -1, 4, 65, 8, one, nullptr) != 0, "unpack_rows: negative n", "negative");
  expect(ape_hip_bitmask_unpack_rows(nullptr, 0, 4, 65, 8, nullptr, nullptr) == 0, "unpack_rows: n = 0", nullptr);

  printf(failures ? "%d FAILED\n" : "boundary_argcheck: all argument checks behave (%d failures)\n", failures);
  return failures ? 1 : 0;
}
