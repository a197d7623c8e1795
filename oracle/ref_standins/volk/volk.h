// functional stand-in (see ../README.md): volk/volk.h — the generic (sequential, one element after the other) form of the
// eight VOLK calls the sink blocks make, in float32, compiled without contraction into fused multiply-adds.
// volk_32f_accumulator_s32f adds in INDEX ORDER; decisions that sit within rounding of a threshold depend on that order.
#pragma once
#include <complex>
#include <cstddef>
typedef std::complex<float> lv_32fc_t;
size_t volk_get_alignment(void);
void *volk_malloc(size_t size, size_t alignment);
void volk_free(void *aptr);
void volk_32fc_x2_multiply_32fc(lv_32fc_t *cVector, const lv_32fc_t *aVector, const lv_32fc_t *bVector, unsigned int num_points);
void volk_32fc_magnitude_squared_32f(float *magnitudeVector, const lv_32fc_t *complexVector, unsigned int num_points);
void volk_32f_x2_divide_32f(float *cVector, const float *aVector, const float *bVector, unsigned int num_points);
void volk_32f_s32f_multiply_32f(float *cVector, const float *aVector, const float scalar, unsigned int num_points);
void volk_32f_accumulator_s32f(float *result, const float *inputBuffer, unsigned int num_points);
