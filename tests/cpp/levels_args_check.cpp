// Stand-alone check of the argument paths of the five channel-level entries (include/fdc_amd.h), meant to be built with the library's HOST code under
// AddressSanitizer + UBSan (tools/levels_san_check.sh) and run on a machine WITHOUT a device: null handles, and a handle whose creation fails with
// FDC_ERR_NO_DEVICE.  With a device present the created handle is exercised through the setting and the accessors without a work call.
#include "../../include/fdc_amd.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

#define EXPECT(cond)                                                         \
    do {                                                                     \
        if (!(cond)) { std::fprintf(stderr, "line %d: %s (last error: %s)\n", __LINE__, #cond, fdc_last_error()); return 1; } \
    } while (0)

int main()
{
    std::vector<float> dst(64, -1.0f);
    // null handles: an argument error each, nothing written
    EXPECT(fdc_pipeline_set_levels(nullptr, 1) == FDC_ERR_INVALID_ARGUMENT);
    EXPECT(fdc_pipeline_set_levels(nullptr, 0) == FDC_ERR_INVALID_ARGUMENT);
    EXPECT(fdc_pipeline_levels(nullptr, dst.data(), 1) == FDC_ERR_INVALID_ARGUMENT);
    EXPECT(fdc_pipeline_levels(nullptr, nullptr, 0) == FDC_ERR_INVALID_ARGUMENT);
    EXPECT(fdc_pipeline_levels_device(nullptr) == nullptr);
    EXPECT(fdc_pipeline_group_set_levels(nullptr, 1) == FDC_ERR_INVALID_ARGUMENT);
    EXPECT(fdc_pipeline_group_levels(nullptr, dst.data(), 1) == FDC_ERR_INVALID_ARGUMENT);
    EXPECT(fdc_pipeline_group_levels(nullptr, nullptr, -1) == FDC_ERR_INVALID_ARGUMENT);
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
        EXPECT(fdc_pipeline_set_levels(p, 1) == FDC_ERR_INVALID_ARGUMENT);
        EXPECT(fdc_pipeline_levels(p, dst.data(), 4) == FDC_ERR_INVALID_ARGUMENT);
        EXPECT(fdc_pipeline_levels_device(p) == nullptr);
        EXPECT(fdc_pipeline_group_set_levels(g, 1) == FDC_ERR_INVALID_ARGUMENT);
        EXPECT(fdc_pipeline_group_levels(g, dst.data(), 4) == FDC_ERR_INVALID_ARGUMENT);
    } else {
        EXPECT(rc == FDC_OK && p && rg == FDC_OK && g);
        EXPECT(fdc_pipeline_levels_device(p) == nullptr);
        EXPECT(fdc_pipeline_levels(p, dst.data(), 4) == FDC_ERR_INVALID_ARGUMENT);          // off
        EXPECT(fdc_pipeline_set_levels(p, 1) == FDC_OK && fdc_pipeline_levels_device(p) != nullptr);
        EXPECT(fdc_pipeline_levels(p, dst.data(), 4) == FDC_ERR_INVALID_ARGUMENT);          // no call yet
        EXPECT(fdc_pipeline_set_levels(p, 0) == FDC_OK && fdc_pipeline_levels_device(p) == nullptr);
        EXPECT(fdc_pipeline_group_levels(g, dst.data(), 4) == FDC_ERR_INVALID_ARGUMENT);
        EXPECT(fdc_pipeline_group_set_levels(g, 1) == FDC_OK);
        EXPECT(fdc_pipeline_group_levels(g, dst.data(), 4) == FDC_ERR_INVALID_ARGUMENT);
        EXPECT(fdc_pipeline_group_set_levels(g, 0) == FDC_OK);
    }
    for (float v : dst) EXPECT(v == -1.0f);
    fdc_pipeline_group_destroy(g);
    fdc_pipeline_destroy(p);
    std::puts("levels_args_check: OK");
    return 0;
}
