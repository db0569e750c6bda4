// Camera helpers shared by the kernels that turn pixels into rays (init_guess.hip: triangulate_kernel, associate.hip:
// assoc_ray_kernel).  The expressions are evaluated under the including file's contraction setting.
#pragma once
#include <hip/hip_runtime.h>

namespace mvfit {

__device__ __forceinline__ void inv3(const double* K, double* Ki) {          // np.linalg.inv of a 3x3
    const double a = K[0], b = K[1], c = K[2], d = K[3], e = K[4], f = K[5], g = K[6], h = K[7], i = K[8];
    const double A = e * i - f * h, B = -(d * i - f * g), C = d * h - e * g;
    const double det = a * A + b * B + c * C;
    const double id = 1.0 / det;
    Ki[0] = A * id;  Ki[1] = -(b * i - c * h) * id; Ki[2] = (b * f - c * e) * id;
    Ki[3] = B * id;  Ki[4] = (a * i - c * g) * id;  Ki[5] = -(a * f - c * d) * id;
    Ki[6] = C * id;  Ki[7] = -(a * h - b * g) * id; Ki[8] = (a * e - b * d) * id;
}

}  // namespace mvfit
