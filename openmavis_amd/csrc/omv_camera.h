// The reference's float camera models (KannalaBrandt8, Pinhole and the GeometricCamera dispatch on the camera type),
// one definition for every float kernel that projects or unprojects: kb8_project_f / kb8_unproject_f, the Pinhole pair
// and cam_project_f / cam_unproject_f.  Their bodies are in omv_math.h beside the libm restatements they call, so that
// the host compiles the same text (oracle/math_host.cpp); this header keeps the name the kernels include.
#pragma once
#include "../../include/omv.h"
#include "omv_device.h"
#include "omv_math.h"
