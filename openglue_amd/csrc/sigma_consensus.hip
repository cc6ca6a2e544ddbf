// Sigma-consensus (MAGSAC++) scoring and weighted refits for the fundamental-matrix and homography RANSAC: what cv2.USAC_MAGSAC
// scores with.
//
//  * og_fundamental_matrix_sc / og_homography_sc are in geometry.hip / homography.hip: the four launches of og_fundamental_matrix /
//    og_homography with the SC = 1 instances of og_ransac_hartley.h's score and finish kernels.  A model's score is Q = sum over its
//    matches of rint(65536 q(e / threshold^2)), the winner the largest Q (lowest model on ties, the same packed atomicMax), the refits
//    are least squares weighted by w and kept when Q does not drop, and `quality` is Q / 65536 of the final model.  q, w and the
//    per-match rule are og_ransac.h's (sigma_consensus, sigma_match).
//
//  * og_sigma_consensus_eval -- sigma_eval_kernel: sigma_consensus over an array of t, as those kernels evaluate it.
#include "og_common.h"
#include "og_ransac.h"

namespace {

__global__ void __launch_bounds__(256) sigma_eval_kernel(int count, const float* t, uint32_t* q, float* w) {
    __shared__ float tab[kSigmaCells + 1];
    sigma_table_fill(tab);
    __syncthreads();
    for (int i = blockIdx.x * 256 + threadIdx.x; i < count; i += gridDim.x * 256) sigma_consensus(tab, t[i], q[i], w[i]);
}

}  // namespace

extern "C" int og_sigma_consensus_eval(int32_t count, const float* t, uint32_t* q, float* w, void* stream) {
    og_clear_status();
    if (count <= 0 || count > (1 << 30) || !t || !q || !w) return OG_E_INVALID;
    const int blocks = (count + 255) / 256;
    hipLaunchKernelGGL(sigma_eval_kernel, dim3(blocks < 1024 ? blocks : 1024), dim3(256), 0, (hipStream_t)stream, count, t, q, w);
    return og_launch_status();
}
