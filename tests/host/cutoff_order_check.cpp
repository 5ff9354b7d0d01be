// Host print-out of the cutoff image's row order and K-step spheres (gpmdm_amd/csrc/host_image.h:
// spatial_order, kstep_spheres -- what capi_model.hip uploads for obs_cutoff.h's tile test), for
// tests/test_cutoff_lists_ref.py to compare its numpy restatement with.  Built by hipcc, run on
// the CPU (no HIP call is made).
//
//   cutoff_order_check FILE      FILE: "N d", then d length scales, then N x d latents, as
//                                C99 hexadecimal floats (exact)
// prints "perm" and N training rows, then "spheres" and ceil(N / 16) x (d + 1) hexadecimal floats.
//
//   cutoff_order_check --chunks  prints, for T_M = 1, 2 and n_act = 0 .. 300 at 32 entries per
//                                chunk, "T_M n_act c* begin(0) .. begin(nc)" (common.h:
//                                cutoff_split_chunk, cutoff_chunk_begin)
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "common.h"
#include "host_image.h"

using namespace gpmdm;

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  if (std::string(argv[1]) == "--chunks") {
    for (int T_M = 1; T_M <= 2; ++T_M)
      for (int n_act = 0; n_act <= 300; ++n_act) {
        const int nt = n_act + T_M, nc = (nt + 31) / 32;
        std::printf("%d %d %d", T_M, n_act, cutoff_split_chunk(n_act, T_M, 32));
        for (int c = 0; c <= nc; ++c) std::printf(" %d", cutoff_chunk_begin(c, nt, 32));
        std::printf("\n");
      }
    std::printf("ok\n");
    return 0;
  }
  std::FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  long long n = 0;
  int d = 0;
  if (std::fscanf(f, "%lld %d", &n, &d) != 2 || n <= 0 || d <= 0 || d > 64) return 2;
  char tok[128];
  auto next = [&](double& v) {
    if (std::fscanf(f, "%127s", tok) != 1) return false;
    v = std::strtod(tok, nullptr);
    return true;
  };
  std::vector<double> ls((size_t)d), X((size_t)n * d);
  for (auto& v : ls)
    if (!next(v)) return 2;
  for (auto& v : X)
    if (!next(v)) return 2;
  std::fclose(f);

  const std::vector<long long> perm = spatial_order(X.data(), ls.data(), n, d);
  std::vector<double> sph;
  kstep_spheres(X.data(), ls.data(), perm.data(), n, d, sph);
  std::printf("perm\n");
  for (long long i = 0; i < n; ++i) std::printf("%lld\n", perm[(size_t)i]);
  std::printf("spheres\n");
  for (size_t i = 0; i < sph.size(); ++i) std::printf("%a\n", sph[i]);
  std::printf("ok\n");
  return 0;
}
