// Stand-alone check of the argument paths of the three channel-gain entries (include/fdc_amd.h), meant to be built with the library's HOST code under
// AddressSanitizer + UBSan (tools/gains_san_check.sh) and run on a machine WITHOUT a device: null handles, bad n, gains that are not finite, and the
// handle a failed create leaves (FDC_ERR_NO_DEVICE).  With a device present the created handles are driven through the setting without a work call.
#include "../../include/fdc_amd.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#define EXPECT(cond)                                                         \
    do {                                                                     \
        if (!(cond)) { std::fprintf(stderr, "line %d: %s (last error: %s)\n", __LINE__, #cond, fdc_last_error()); return 1; } \
    } while (0)

int main()
{
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    std::vector<float> dst(8, -1.0f);
    const float good[2] = {2.5f, -0.125f}, with_nan[2] = {1.0f, nan}, with_inf[2] = {-inf, 1.0f}, ones[2] = {1.0f, 1.0f};
    // null handles: an argument error each, nothing written, whatever the other arguments
    EXPECT(fdc_pipeline_set_gains(nullptr, good, 2) == FDC_ERR_INVALID_ARGUMENT);
    EXPECT(fdc_pipeline_set_gains(nullptr, nullptr, 0) == FDC_ERR_INVALID_ARGUMENT);
    EXPECT(fdc_pipeline_set_gains(nullptr, with_nan, -1) == FDC_ERR_INVALID_ARGUMENT);
    EXPECT(fdc_pipeline_gains(nullptr, dst.data(), 2) == FDC_ERR_INVALID_ARGUMENT);
    EXPECT(fdc_pipeline_gains(nullptr, nullptr, 0) == FDC_ERR_INVALID_ARGUMENT);
    EXPECT(fdc_pipeline_group_set_gains(nullptr, good, 2) == FDC_ERR_INVALID_ARGUMENT);
    EXPECT(fdc_pipeline_group_set_gains(nullptr, nullptr, 0) == FDC_ERR_INVALID_ARGUMENT);
    for (float v : dst) EXPECT(v == -1.0f);

    fdc_channel ch[2] = {{100, 256, 0.8, 1.0}, {700, 512, 0.75, 0.95}};
    fdc_pipeline_cfg cfg{};
    cfg.device_id = 0; cfg.blocklen = 4096; cfg.relinvovl = 2; cfg.windowtype = 1; cfg.nchannels = 2; cfg.channels = ch; cfg.max_blocks = 4;
    fdc_pipeline *p = nullptr;
    fdc_pipeline_group *g = nullptr;
    const int32_t devs[2] = {0, 0};
    const int rc = fdc_pipeline_create(&cfg, &p);
    const int rg = fdc_pipeline_group_create(&cfg, devs, 2, 2, &g);
    if (fdc_device_count() < 1) {
        // no device: the creation fails loudly and leaves no handle; the entries see the null it left
        EXPECT(rc == FDC_ERR_NO_DEVICE && p == nullptr);
        EXPECT(rg == FDC_ERR_NO_DEVICE && g == nullptr);
        EXPECT(fdc_pipeline_set_gains(p, good, 2) == FDC_ERR_INVALID_ARGUMENT);
        EXPECT(fdc_pipeline_set_gains(p, with_inf, 2) == FDC_ERR_INVALID_ARGUMENT);
        EXPECT(fdc_pipeline_set_gains(p, good, 3) == FDC_ERR_INVALID_ARGUMENT);
        EXPECT(fdc_pipeline_gains(p, dst.data(), 2) == FDC_ERR_INVALID_ARGUMENT);
        EXPECT(fdc_pipeline_group_set_gains(g, good, 2) == FDC_ERR_INVALID_ARGUMENT);
        EXPECT(fdc_pipeline_group_set_gains(g, with_nan, 2) == FDC_ERR_INVALID_ARGUMENT);
        for (float v : dst) EXPECT(v == -1.0f);
    } else {
        EXPECT(rc == FDC_OK && p && rg == FDC_OK && g);
        EXPECT(fdc_pipeline_gains(p, dst.data(), 2) == FDC_OK && dst[0] == 1.0f && dst[1] == 1.0f && dst[2] == -1.0f);      // off: ones
        EXPECT(fdc_pipeline_gains(p, dst.data(), 3) == FDC_ERR_INVALID_ARGUMENT && dst[2] == -1.0f);
        EXPECT(fdc_pipeline_gains(p, nullptr, 2) == FDC_ERR_INVALID_ARGUMENT);
        EXPECT(fdc_pipeline_set_gains(p, good, 1) == FDC_ERR_INVALID_ARGUMENT);
        EXPECT(fdc_pipeline_set_gains(p, good, 3) == FDC_ERR_INVALID_ARGUMENT);
        EXPECT(fdc_pipeline_set_gains(p, nullptr, 0) == FDC_ERR_INVALID_ARGUMENT);
        EXPECT(fdc_pipeline_set_gains(p, good, 2) == FDC_OK);
        EXPECT(fdc_pipeline_set_gains(p, with_nan, 2) == FDC_ERR_INVALID_ARGUMENT);
        EXPECT(fdc_pipeline_set_gains(p, with_inf, 2) == FDC_ERR_INVALID_ARGUMENT);
        EXPECT(fdc_pipeline_gains(p, dst.data(), 2) == FDC_OK && dst[0] == good[0] && dst[1] == good[1]);                  // the previous gains hold
        EXPECT(fdc_pipeline_set_gains(p, ones, 2) == FDC_OK);
        EXPECT(fdc_pipeline_gains(p, dst.data(), 2) == FDC_OK && dst[0] == 1.0f && dst[1] == 1.0f);
        EXPECT(fdc_pipeline_set_gains(p, good, 2) == FDC_OK && fdc_pipeline_set_gains(p, nullptr, 2) == FDC_OK);
        EXPECT(fdc_pipeline_group_set_gains(g, good, 3) == FDC_ERR_INVALID_ARGUMENT);
        EXPECT(fdc_pipeline_group_set_gains(g, with_nan, 2) == FDC_ERR_INVALID_ARGUMENT);
        EXPECT(fdc_pipeline_group_set_gains(g, good, 2) == FDC_OK);
        EXPECT(fdc_pipeline_gains(fdc_pipeline_group_member(g, 1), dst.data(), 2) == FDC_OK && dst[0] == good[0] && dst[1] == good[1]);
        EXPECT(fdc_pipeline_group_set_gains(g, nullptr, 2) == FDC_OK);
    }
    fdc_pipeline_group_destroy(g);
    fdc_pipeline_destroy(p);
    std::puts("gains_args_check: OK");
    return 0;
}
