// la_gemm_pp_cp_f16.hip -- the cache-policy instantiations of the 256 x 256 GEMM kernel (la_gemm_pp_kernel.h gemm_pp_kernel_cp; options
// cp_epi16, cp_split_st, cp_split_ld, cp_gemm_a) for IEEE half operands: a translation unit of their own, compiled beside the default kernels'.
#include "la_gemm_pp_kernel.h"

namespace la {
namespace gemm {

int launch_pp_cp_f16(GemmParams p, int batch, int lnm, bool duo, int cp, hipStream_t stream) { return launch_pp_cp<la::f16_t>(p, batch, lnm, duo, cp, stream); }

}  // namespace gemm
}  // namespace la
