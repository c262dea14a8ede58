// test_bow_angle.cpp -- csrc/bow_angle.h (the bin of a pair of angles, the three-bin choice of ORBMatcher::verifyAngle) with the host
// compiler alone: the same text k_bowsearch.hip compiles for the device.  Reads the cases the Python restatement
// (frontend.ORBMatcher.verifyAngle's rules) wrote:
//   P <angle_q bits> <angle_t bits> <bin>              the float32 bit patterns in hex, so that no decimal round trip is involved
//   C <30 counts> <mask of the chosen bins>
// Prints OK <pairs> <choices>, or the first difference.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "bow_angle.h"

static float from_bits(unsigned long v) {
  const uint32_t u = (uint32_t)v;
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  char kind[4];
  long pairs = 0, choices = 0;
  while (std::fscanf(f, "%3s", kind) == 1) {
    if (kind[0] == 'P') {
      unsigned long a, b;
      int want;
      if (std::fscanf(f, "%lx %lx %d", &a, &b, &want) != 3) return 2;
      const int got = bow_angle_bin(from_bits(a), from_bits(b));
      if (got != want || got < 0 || got >= BOW_ANGLE_BINS) {
        std::printf("bin of (%lx, %lx): %d, expected %d\n", a, b, got, want);
        return 1;
      }
      ++pairs;
    } else if (kind[0] == 'C') {
      int32_t* count = (int32_t*)std::malloc(BOW_ANGLE_BINS * sizeof(int32_t));  // exactly 30: a read past the bins is a sanitizer error
      for (int i = 0; i < BOW_ANGLE_BINS; ++i)
        if (std::fscanf(f, "%d", &count[i]) != 1) return 2;
      unsigned long want;
      if (std::fscanf(f, "%lx", &want) != 1) return 2;
      const uint32_t got = bow_angle_choose(count);
      std::free(count);
      if (got != (uint32_t)want) {
        std::printf("choice %ld: mask %x, expected %lx\n", choices, got, want);
        return 1;
      }
      ++choices;
    } else
      return 2;
  }
  std::fclose(f);
  std::printf("OK %ld %ld\n", pairs, choices);
  return 0;
}
