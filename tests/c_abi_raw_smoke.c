/* C-only client of libvgh.so on images of ANY size (no Python, no torch, no letterbox tables): vgh_create from a .vghpack, raw u8
 * images of different sizes uploaded as they are, one vgh_ctx_detect(..., VGH_IMG_U8_RAW, ...), the detector's un-pad table read through
 * VGH_SCRATCH_UNPAD; every result written as raw little-endian arrays.  tests/test_gpu_raw_images.py::test_c_only_client_on_raw_images
 * compiles this with plain gcc, runs it and compares the bytes with the Python path.
 *   c_abi_raw_smoke <pack> <images.bin> <B> <conf> <out_prefix>
 * images.bin: B records of {int32 h, w, channels; int64 pitch_bytes; h * pitch_bytes pixel bytes}. */
#include <hip/hip_runtime_api.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "vgh.h"

#define CHECK_HIP(e)                                                                            \
    do {                                                                                        \
        hipError_t _e = (e);                                                                    \
        if (_e != hipSuccess) {                                                                 \
            fprintf(stderr, "%s:%d hip error %s\n", __FILE__, __LINE__, hipGetErrorString(_e)); \
            return 2;                                                                           \
        }                                                                                       \
    } while (0)

static int dump(const char* prefix, const char* name, const void* dev, size_t bytes) {
    char path[1024];
    void* host = malloc(bytes ? bytes : 1);
    FILE* f;
    if (hipMemcpy(host, dev, bytes, hipMemcpyDeviceToHost) != hipSuccess) return 1;
    snprintf(path, sizeof(path), "%s.%s", prefix, name);
    f = fopen(path, "wb");
    if (!f) return 1;
    fwrite(host, 1, bytes, f);
    fclose(f);
    free(host);
    return 0;
}

int main(int argc, char** argv) {
    vgh_config cfg;
    vgh_ctx* ctx = NULL;
    vgh_ctx_info info;
    vgh_detect_out out;
    vgh_raw_image* imgs;
    int B, rc, cap, i;
    float conf;
    FILE* f;
    const float* unpad;
    if (argc != 6) {
        fprintf(stderr, "usage: %s pack images.bin B conf out_prefix\n", argv[0]);
        return 1;
    }
    if (vgh_abi_version() != VGH_ABI_VERSION) {
        fprintf(stderr, "libvgh.so has ABI revision %d, vgh.h %d\n", vgh_abi_version(), VGH_ABI_VERSION);
        return 1;
    }
    B = atoi(argv[3]);
    conf = (float)atof(argv[4]);
    memset(&cfg, 0, sizeof(cfg));
    cfg.device = 0;
    cfg.pack_path = argv[1];
    cfg.max_batch = B;
    rc = vgh_create(&cfg, &ctx);
    if (rc != VGH_OK) {
        fprintf(stderr, "vgh_create failed (%d): %s\n", rc, vgh_last_error());
        return 3;
    }
    if (vgh_ctx_get_info(ctx, &info) != VGH_OK) return 3;
    /* the images as they are: each in its own device allocation, rows pitch_bytes apart */
    imgs = (vgh_raw_image*)calloc((size_t)B, sizeof(vgh_raw_image));
    f = fopen(argv[2], "rb");
    if (!f) return 1;
    for (i = 0; i < B; ++i) {
        int32_t hwc[3];
        int64_t pitch;
        size_t bytes;
        void *host, *dev;
        if (fread(hwc, 4, 3, f) != 3 || fread(&pitch, 8, 1, f) != 1) return 1;
        bytes = (size_t)hwc[0] * (size_t)pitch;
        host = malloc(bytes);
        if (fread(host, 1, bytes, f) != bytes) return 1;
        CHECK_HIP(hipMalloc(&dev, bytes));
        CHECK_HIP(hipMemcpy(dev, host, bytes, hipMemcpyHostToDevice));
        free(host);
        imgs[i].data_dev = (const uint8_t*)dev;
        imgs[i].h = hwc[0];
        imgs[i].w = hwc[1];
        imgs[i].channels = hwc[2];
        imgs[i].pitch_bytes = pitch;
        printf("image %d: %d x %d x %d, pitch %lld\n", i, hwc[0], hwc[1], hwc[2], (long long)pitch);
    }
    fclose(f);
    cap = B * info.keep_top_k;
    memset(&out, 0, sizeof(out));
    CHECK_HIP(hipMalloc((void**)&out.boxes_dev, (size_t)cap * 4 * 4));
    CHECK_HIP(hipMalloc((void**)&out.scores_dev, (size_t)cap * 4));
    CHECK_HIP(hipMalloc((void**)&out.flame_dev, (size_t)cap * VGH_NUM_FLAME_PARAMS * 4));
    CHECK_HIP(hipMalloc((void**)&out.counts_dev, (size_t)B * 4));
    CHECK_HIP(hipMalloc((void**)&out.n_heads_dev, 4));
    CHECK_HIP(hipMalloc((void**)&out.head_image_dev, (size_t)cap * 4));
    CHECK_HIP(hipMalloc((void**)&out.rpy_dev, (size_t)cap * 3 * 4));
    CHECK_HIP(hipMalloc((void**)&out.proj_dev, (size_t)cap * info.num_vertices * 3 * 4));
    CHECK_HIP(hipMemset(out.proj_dev, 0, (size_t)cap * info.num_vertices * 3 * 4));
    CHECK_HIP(hipMemset(out.rpy_dev, 0, (size_t)cap * 3 * 4));
    CHECK_HIP(hipMemset(out.head_image_dev, 0, (size_t)cap * 4));
    out.head_capacity = cap;
    out.unpad_dev = NULL; /* RAW: the FLAME outputs are un-padded with the detector's own table */
    /* an invalid descriptor fails before anything is queued, naming the image */
    {
        const uint8_t* keep = imgs[B - 1].data_dev;
        char want[64];
        imgs[B - 1].data_dev = NULL;
        snprintf(want, sizeof(want), "image %d", B - 1);
        if (vgh_ctx_detect(ctx, imgs, VGH_IMG_U8_RAW, B, conf, 0.5f, &out, NULL) != VGH_ERR_INVALID || !strstr(vgh_ctx_last_error(ctx), want)) {
            fprintf(stderr, "expected a NULL data_dev to fail naming %s, got: %s\n", want, vgh_ctx_last_error(ctx));
            return 4;
        }
        imgs[B - 1].data_dev = keep;
    }
    if (vgh_detector_scratch(vgh_ctx_detector(ctx), VGH_SCRATCH_UNPAD) != NULL) {
        fprintf(stderr, "the un-pad table exists before the first RAW call\n");
        return 4;
    }
    rc = vgh_ctx_detect(ctx, imgs, VGH_IMG_U8_RAW, B, conf, 0.5f, &out, NULL);
    if (rc != VGH_OK) {
        fprintf(stderr, "vgh_ctx_detect failed (%d): %s\n", rc, vgh_ctx_last_error(ctx));
        return 4;
    }
    CHECK_HIP(hipDeviceSynchronize());
    unpad = (const float*)vgh_detector_scratch(vgh_ctx_detector(ctx), VGH_SCRATCH_UNPAD);
    if (!unpad) {
        fprintf(stderr, "VGH_SCRATCH_UNPAD is NULL after a RAW call\n");
        return 4;
    }
    if (dump(argv[5], "counts", out.counts_dev, (size_t)B * 4) || dump(argv[5], "boxes", out.boxes_dev, (size_t)cap * 16) || dump(argv[5], "scores", out.scores_dev, (size_t)cap * 4) ||
        dump(argv[5], "flame", out.flame_dev, (size_t)cap * VGH_NUM_FLAME_PARAMS * 4) || dump(argv[5], "n_heads", out.n_heads_dev, 4) ||
        dump(argv[5], "head_image", out.head_image_dev, (size_t)cap * 4) || dump(argv[5], "rpy", out.rpy_dev, (size_t)cap * 12) ||
        dump(argv[5], "proj", out.proj_dev, (size_t)cap * info.num_vertices * 12) || dump(argv[5], "unpad", unpad, (size_t)B * 12))
        return 5;
    vgh_destroy(ctx);
    for (i = 0; i < B; ++i) hipFree((void*)imgs[i].data_dev);
    free(imgs);
    printf("ok\n");
    return 0;
}
