// Host-only check of the "kept positions" entries' argument validation (include/talkshow_hip.h): every call below must be refused before
// anything touches a device, so the program runs on a machine without a GPU.  Meant to be built with the host sanitizers, e.g.
//   make -C talkshow_amd/csrc CXXFLAGS="--offload-arch=gfx950 -O1 -g -std=c++17 -fPIC -Xarch_host -fsanitize=address,undefined" OUT=$PWD/san/libts_san.so
//   clang++ -std=c++17 -g -fsanitize=address,undefined -Iinclude tools/keep_args_check.cpp -Lsan -lts_san -Wl,-rpath,$PWD/san -o san/keep_args_check
// (in a copy of the tree, so that the objects of the product build stay as they are) and run as it is: exit status 0 and "ok" on success.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "talkshow_hip.h"

static int failures = 0;

static void refused(const char *what, int rc, const char *needle) {
    const char *msg = ts_last_error();
    const bool ok = rc != 0 && msg && std::strstr(msg, needle);
    std::printf("%-64s rc=%d %s\n", what, rc, ok ? "refused as expected" : "NOT REFUSED AS EXPECTED");
    if (!ok) {
        std::printf("    message: %s (wanted \"%s\")\n", msg ? msg : "(none)", needle);
        ++failures;
    }
}

int main() {
    // stand-ins for handles and device pointers: the entries must not dereference any of them on these paths
    alignas(16) static unsigned char blob[256];
    auto *ae = reinterpret_cast<ts_convnet *>(blob);
    auto *pix = reinterpret_cast<ts_pixelcnn *>(blob);
    auto *vq = reinterpret_cast<ts_vqvae *>(blob);
    auto *ctx = reinterpret_cast<ts_ctx *>(blob);
    const float *f = reinterpret_cast<const float *>(blob);
    const int64_t *i64 = reinterpret_cast<const int64_t *>(blob);
    int64_t *codes = reinterpret_cast<int64_t *>(blob);
    float *poses = reinterpret_cast<float *>(blob);
    const uint8_t *keep = blob;
    const int B = 3, T_max = 40, H = 10;
    const std::vector<int32_t> lens = {40, 24, 8}, lens_dev_standin = {40, 24, 8};
    const int32_t *ld = lens_dev_standin.data();
    const std::vector<int32_t> g_ok = {10, 0, 2}, g_long = {10, 7, 2}, g_neg = {10, 0, -1}, p_short = {40, 3, 0}, p_long = {40, 28, 0}, p_ok = {40, 0, 8},
                               unsorted = {24, 40, 8};

    // ---- ts_pixelcnn_generate_mixed_keep ----
    refused("chain: null handle", ts_pixelcnn_generate_mixed_keep(nullptr, i64, f, lens.data(), ld, B, H, TS_SAMPLE_GREEDY, nullptr, 0, nullptr, codes,
                                                                  nullptr, 0, nullptr, i64, g_ok.data(), nullptr, keep, nullptr), "null argument");
    refused("chain: mask without given codes", ts_pixelcnn_generate_mixed_keep(pix, i64, f, lens.data(), ld, B, H, TS_SAMPLE_GREEDY, nullptr, 0, nullptr,
                                                                               codes, nullptr, 0, nullptr, nullptr, nullptr, nullptr, keep, nullptr),
            "needs the given codes");
    refused("chain: given codes without their table", ts_pixelcnn_generate_mixed_keep(pix, i64, f, lens.data(), ld, B, H, TS_SAMPLE_GREEDY, nullptr, 0,
                                                                                      nullptr, codes, nullptr, 0, nullptr, i64, nullptr, nullptr, keep,
                                                                                      nullptr), "row table");
    refused("chain: G_b > H_b", ts_pixelcnn_generate_mixed_keep(pix, i64, f, lens.data(), ld, B, H, TS_SAMPLE_GREEDY, nullptr, 0, nullptr, codes, nullptr,
                                                                0, nullptr, i64, g_long.data(), nullptr, keep, nullptr), "clip 1");
    refused("chain: G_b < 0", ts_pixelcnn_generate_mixed_keep(pix, i64, f, lens.data(), ld, B, H, TS_SAMPLE_GREEDY, nullptr, 0, nullptr, codes, nullptr, 0,
                                                              nullptr, i64, g_neg.data(), nullptr, keep, nullptr), "clip 2");
    refused("chain: uniforms mode without uniforms", ts_pixelcnn_generate_mixed_keep(pix, i64, f, lens.data(), ld, B, H, TS_SAMPLE_UNIFORMS, nullptr, 0,
                                                                                     nullptr, codes, nullptr, 0, nullptr, i64, g_ok.data(), nullptr, keep,
                                                                                     nullptr), "uniforms required");
    refused("chain: bad mode", ts_pixelcnn_generate_mixed_keep(pix, i64, f, lens.data(), ld, B, H, 77, nullptr, 0, nullptr, codes, nullptr, 0, nullptr, i64,
                                                               g_ok.data(), nullptr, keep, nullptr), "bad mode");
    // ---- ts_body_pixel_infer_mixed_keep ----
    refused("body: null handle", ts_body_pixel_infer_mixed_keep(nullptr, pix, vq, vq, f, i64, lens.data(), ld, B, T_max, TS_SAMPLE_GREEDY, nullptr, 0,
                                                                nullptr, codes, poses, nullptr, 0, nullptr, i64, g_ok.data(), nullptr, keep, nullptr),
            "null argument");
    refused("body: mask without given codes", ts_body_pixel_infer_mixed_keep(ae, pix, vq, vq, f, i64, lens.data(), ld, B, T_max, TS_SAMPLE_GREEDY, nullptr,
                                                                             0, nullptr, codes, poses, nullptr, 0, nullptr, nullptr, nullptr, nullptr, keep,
                                                                             nullptr), "needs the given codes");
    refused("body: G_b > H_b", ts_body_pixel_infer_mixed_keep(ae, pix, vq, vq, f, i64, lens.data(), ld, B, T_max, TS_SAMPLE_GREEDY, nullptr, 0, nullptr,
                                                              codes, poses, nullptr, 0, nullptr, i64, g_long.data(), nullptr, keep, nullptr), "clip 1");
    refused("body: lengths not sorted", ts_body_pixel_infer_mixed_keep(ae, pix, vq, vq, f, i64, unsorted.data(), ld, B, T_max, TS_SAMPLE_GREEDY, nullptr, 0,
                                                                       nullptr, codes, poses, nullptr, 0, nullptr, i64, g_ok.data(), nullptr, keep, nullptr),
            "clip 1 is longer than the one before it");
    // ---- ts_body_pixel_infer_mixed_poses_keep ----
    refused("poses: mask without given poses", ts_body_pixel_infer_mixed_poses_keep(ae, pix, vq, vq, f, i64, lens.data(), ld, B, T_max, TS_SAMPLE_GREEDY,
                                                                                    nullptr, 0, nullptr, codes, poses, nullptr, 0, nullptr, nullptr, 0,
                                                                                    nullptr, nullptr, keep, nullptr), "needs the given poses");
    refused("poses: no frame tables", ts_body_pixel_infer_mixed_poses_keep(ae, pix, vq, vq, f, i64, lens.data(), ld, B, T_max, TS_SAMPLE_GREEDY, nullptr, 0,
                                                                           nullptr, codes, poses, nullptr, 0, nullptr, f, 40, nullptr, nullptr, keep,
                                                                           nullptr), "frame tables");
    refused("poses: 1 <= P_b <= 3", ts_body_pixel_infer_mixed_poses_keep(ae, pix, vq, vq, f, i64, lens.data(), ld, B, T_max, TS_SAMPLE_GREEDY, nullptr, 0,
                                                                         nullptr, codes, poses, nullptr, 0, nullptr, f, 40, p_short.data(), ld, keep,
                                                                         nullptr), "clip 1");
    refused("poses: more code rows than the clip has", ts_body_pixel_infer_mixed_poses_keep(ae, pix, vq, vq, f, i64, lens.data(), ld, B, T_max,
                                                                                            TS_SAMPLE_GREEDY, nullptr, 0, nullptr, codes, poses, nullptr, 0,
                                                                                            nullptr, f, 40, p_long.data(), ld, keep, nullptr), "clip 1");
    refused("poses: a clip brings more frames than P_max", ts_body_pixel_infer_mixed_poses_keep(ae, pix, vq, vq, f, i64, lens.data(), ld, B, T_max,
                                                                                                TS_SAMPLE_GREEDY, nullptr, 0, nullptr, codes, poses, nullptr,
                                                                                                0, nullptr, f, 16, p_ok.data(), ld, keep, nullptr), "P_max");
    // ---- ts_op_sample_keep ----
    refused("op: null context", ts_op_sample_keep(nullptr, f, B, 8, TS_SAMPLE_GREEDY, nullptr, 0, 0, 3, nullptr, 0, codes, nullptr, g_ok.data(), keep, i64,
                                                  nullptr), "null argument");
    refused("op: no row table", ts_op_sample_keep(ctx, f, B, 8, TS_SAMPLE_GREEDY, nullptr, 0, 0, 3, nullptr, 0, codes, nullptr, nullptr, keep, i64, nullptr),
            "null argument");
    refused("op: bad shape", ts_op_sample_keep(ctx, f, 0, 8, TS_SAMPLE_GREEDY, nullptr, 0, 0, 3, nullptr, 0, codes, nullptr, g_ok.data(), keep, i64, nullptr),
            "bad shape");
    refused("op: teacher forcing is not a given mode", ts_op_sample_keep(ctx, f, B, 8, TS_TEACHER_FORCED, nullptr, 0, 0, 3, nullptr, 0, codes, nullptr,
                                                                         g_ok.data(), keep, i64, nullptr), "bad mode");
    refused("op: uniforms mode without uniforms", ts_op_sample_keep(ctx, f, B, 8, TS_SAMPLE_UNIFORMS, nullptr, 0, 0, 3, nullptr, 0, codes, nullptr,
                                                                    g_ok.data(), keep, i64, nullptr), "uniforms required");
    refused("op: position too large", ts_op_sample_keep(ctx, f, B, 8, TS_SAMPLE_GREEDY, nullptr, 0, 0, 0x7ffffff1u, nullptr, 0, codes, nullptr, g_ok.data(),
                                                        keep, i64, nullptr), "position too large");
    refused("op: negative row count", ts_op_sample_keep(ctx, f, B, 8, TS_SAMPLE_GREEDY, nullptr, 0, 0, 3, nullptr, 0, codes, nullptr, g_neg.data(), keep,
                                                        i64, nullptr), "row 2");
    ts_sampling rec;
    rec.temperature = 1.0f; rec.top_p = 1.0f; rec.top_k = 0; rec.reserved = 0;
    refused("op: a record with greedy", ts_op_sample_keep(ctx, f, B, 8, TS_SAMPLE_GREEDY, nullptr, 0, 0, 3, &rec, 1, codes, nullptr, g_ok.data(), keep, i64,
                                                          nullptr), "top_k = 1");
    std::printf(failures ? "%d check(s) FAILED\n" : "ok (%d failures)\n", failures);
    return failures ? 1 : 0;
}
