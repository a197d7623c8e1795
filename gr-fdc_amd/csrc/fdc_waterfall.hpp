// The waterfall's data path (fdc_waterfall.hip) as the pipeline entry (fdc_api.hip, fdc_pipeline_work_waterfall) uses it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/fdc_amd.h"

namespace fdc {

constexpr int kWfWidth = 1024;    // pixels per row (python/WaterfallMsgTagging.py:43 normwidth)

// checks that w can take nblocks blocks of length N on device_id and that at most cap_rows rows finish; returns FDC_OK or a status
int wf_check_call(const fdc_waterfall *w, int device_id, int N, int nblocks, int cap_rows);
// the [nblocks][1024] row sums of the call: the fused kernel writes them, or one of the two launchers below
float *wf_block_rows(fdc_waterfall *w);
// nblocks x N/16 floats for the 16-bin group powers of the call (allocated at the first use: no allocation in the steady state)
int wf_group_buffer(fdc_waterfall *w, int nblocks, float **out);
hipError_t wf_rows_from_spectrum(fdc_waterfall *w, const float2 *spec, int nblocks, hipStream_t s);
hipError_t wf_rows_from_groups(fdc_waterfall *w, const float *gpow, int nblocks, hipStream_t s);
// the call's blocks are in wf_block_rows(w) (enqueued on s): decimation, colours, copies to the caller's buffers, synchronisation
int wf_finish(fdc_waterfall *w, int nblocks, hipStream_t s, float *rows, uint16_t *index, uint8_t *rgb, int32_t *nrows);

}  // namespace fdc
