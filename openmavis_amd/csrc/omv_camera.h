// The reference's float camera models (KannalaBrandt8, Pinhole and the GeometricCamera dispatch on the camera type),
// one definition for every float kernel that projects or unprojects.  Float arithmetic without contraction, in the
// reference's operation order; glibc's atan2f / tanf and the correctly rounded sqrtf are the restatements of
// omv_device.h.  The double-precision model of the g2o edges (g2o_types.h) is a different function of the reference.
#pragma once
#include "../../include/omv.h"
#include "omv_device.h"

namespace omv {

// KannalaBrandt8::project(const Eigen::Vector3f&) (KannalaBrandt8.cpp:48-67): cos / sin of the promoted float
// (C double functions)
__device__ __forceinline__ void kb8_project_f(const float *k, const float *X, float &u, float &v) {
    const float x2y2 = X[0] * X[0] + X[1] * X[1];
    const float theta = omv::glibc_atan2f(omv::sqrtf_cr(x2y2), X[2]);
    const float psi = omv::glibc_atan2f(X[1], X[0]);
    const float t2 = theta * theta, t3 = theta * t2, t5 = t3 * t2, t7 = t5 * t2, t9 = t7 * t2;
    const float r = theta + k[4] * t3 + k[5] * t5 + k[6] * t7 + k[7] * t9;
    u = (float)((double)(k[0] * r) * cos((double)psi) + (double)k[2]);
    v = (float)((double)(k[1] * r) * sin((double)psi) + (double)k[3]);
}

// KannalaBrandt8::unproject (precision 1e-6, <= 10 Newton steps, scale = std::tan(theta) / theta_d)
__device__ __forceinline__ void kb8_unproject_f(const float *k, float px, float py, float *ray) {
    const float pwx = (px - k[2]) / k[0], pwy = (py - k[3]) / k[1];
    float scale = 1.f;
    float theta_d = omv::sqrtf_cr(pwx * pwx + pwy * pwy);
    theta_d = fminf(fmaxf((float)(-3.14159265358979323846 / 2.f), theta_d), (float)(3.14159265358979323846 / 2.f));
    if ((double)theta_d > 1e-8) {
        float theta = theta_d;
        for (int j = 0; j < 10; j++) {
            const float theta2 = theta * theta, theta4 = theta2 * theta2, theta6 = theta4 * theta2,
                        theta8 = theta4 * theta4;
            const float k0_theta2 = k[4] * theta2, k1_theta4 = k[5] * theta4;
            const float k2_theta6 = k[6] * theta6, k3_theta8 = k[7] * theta8;
            const float theta_fix = (theta * (1 + k0_theta2 + k1_theta4 + k2_theta6 + k3_theta8) - theta_d) /
                                    (1 + 3 * k0_theta2 + 5 * k1_theta4 + 7 * k2_theta6 + 9 * k3_theta8);
            theta = theta - theta_fix;
            if (fabsf(theta_fix) < 1e-6f) break;
        }
        scale = omv::glibc_tanf(theta) / theta_d;
    }
    ray[0] = pwx * scale, ray[1] = pwy * scale, ray[2] = 1.f;
}

// Pinhole::unprojectEig / project(const Eigen::Vector3f&) (Pinhole.cpp:26-32, :40-45): float, left to right
__device__ __forceinline__ void pinhole_unproject_f(const float *k, float px, float py, float *ray) {
    ray[0] = (px - k[2]) / k[0], ray[1] = (py - k[3]) / k[1], ray[2] = 1.f;
}
__device__ __forceinline__ void pinhole_project_f(const float *k, const float *X, float &u, float &v) {
    u = k[0] * X[0] / X[2] + k[2];
    v = k[1] * X[1] / X[2] + k[3];
}
// GeometricCamera::unprojectEig / project, dispatched on the camera type (the virtual calls of
// KannalaBrandt8::TriangulateMatches on pCamera2, KannalaBrandt8.cpp:330, :382)
__device__ __forceinline__ void cam_unproject_f(int model, const float *k, float px, float py, float *ray) {
    if (model == OMV_CAM_PINHOLE) pinhole_unproject_f(k, px, py, ray);
    else kb8_unproject_f(k, px, py, ray);
}
__device__ __forceinline__ void cam_project_f(int model, const float *k, const float *X, float &u, float &v) {
    if (model == OMV_CAM_PINHOLE) pinhole_project_f(k, X, u, v);
    else kb8_project_f(k, X, u, v);
}

}  // namespace omv
