// Device audio front-end: waveform -> (resample to 22 kHz) -> MFCC(64) as the reference computes it on the CPU with
// torchaudio (data_utils/utils.py:148-231: Resample(sr_0, 22000) per channel, MFCC(n_mfcc=64, n_fft=2048, n_mels=256,
// hop=734|1467, mel_scale='htk')).  torchaudio is third-party and not available in this image: the constants below
// restate its published definitions (sinc_interp_hann kernel with lowpass_filter_width 6 / rolloff 0.99; periodic Hann;
// HTK mel filterbank f_min 0, f_max sr/2, norm None; 10*log10(clamp 1e-10), top_db 80 per clip; orthonormal DCT-II).
// PARITY UNPINNED against torchaudio; pinned against talkshow_amd/frontend.py (same formulae in numpy) on the GPU.
// The STFT is one kernel (framing + window + a radix-4 Stockham real FFT in LDS + |X|^2, mfcc.hip); the mel projection and the
// DCT are GEMMs on conv_gemm_f32.  (Rounds 1-3 ran the transform as a 2048 x 2050 DFT matrix: 1.26 GMAC per 10 s clip.)
#include <cmath>
#include <mutex>

#include "host_common.h"

using namespace ts;

struct ts_mfcc {
    ts_ctx *ctx = nullptr;
    int sr_in = 0, sr_out = 0, norig = 1, nnew = 1, width = 0, kw = 0;
    int nfft = 2048, hop = 734, nmels = 256, nmfcc = 64, nbins = 1025, nbins_pad = 1056;
    DevBuf rs_kern, window, tw1024, tw2048;   // FFT twiddles: exp(-2 pi i m / 1024), m < 1024; exp(-2 pi i k / 2048), k <= 1024
    ConvLayer mel, dct;
    struct Work {
        DevBuf x22, power, melb;
        DevBuf frames;   // mixed passes: the recordings' own frame counts (the row table of the masked GEMMs), written on the stream by every call
    };
    StreamWorks<Work> works;
    Work &work(hipStream_t s) { return works.get(s); }
    long resampled_len(long N) const { return (nnew * N + norig - 1) / norig; }
};

static int gcd_i(int a, int b) { return b ? gcd_i(b, a % b) : a; }

extern "C" {

int ts_mfcc_create(ts_ctx *ctx, int sr_in, int sr_out, int fps, ts_mfcc **out) {
    if (!ctx || !out) return fail("ts_mfcc_create: null argument");
    if (fps != 30 && fps != 15) return fail("ts_mfcc_create: fps must be 15 or 30 (hop 1467 / 734, utils.py:157-160)");
    TS_HIP(hipSetDevice(ctx->device));
    std::unique_ptr<ts_mfcc> m(new ts_mfcc());
    m->ctx = ctx;
    m->sr_in = sr_in;
    m->sr_out = sr_out;
    m->hop = fps == 30 ? 734 : 1467;
    const double PI = 3.14159265358979323846;
    // ---- resampling kernel (torchaudio _get_sinc_resample_kernel, sinc_interp_hann) ----
    if (sr_in != sr_out) {
        const int g = gcd_i(sr_in, sr_out);
        m->norig = sr_in / g;
        m->nnew = sr_out / g;
        const double lpw = 6.0, rolloff = 0.99;
        const double base = std::min(m->norig, m->nnew) * rolloff;
        m->width = (int)std::ceil(lpw * m->norig / base);
        m->kw = 2 * m->width + m->norig;
        std::vector<float> k((size_t)m->nnew * m->kw);
        for (int ph = 0; ph < m->nnew; ++ph)
            for (int i = 0; i < m->kw; ++i) {
                double t = ((double)(-ph) / m->nnew + (double)(i - m->width) / m->norig) * base;
                t = std::max(-lpw, std::min(lpw, t));
                const double win = std::pow(std::cos(t * PI / lpw / 2.0), 2.0);
                const double tp = t * PI;
                const double sinc = tp == 0.0 ? 1.0 : std::sin(tp) / tp;
                k[(size_t)ph * m->kw + i] = (float)(sinc * win * (base / m->norig));
            }
        TS_TRY(m->rs_kern.upload(k.data(), k.size() * sizeof(float)));
    }
    // ---- periodic Hann window ----
    {
        std::vector<float> w(m->nfft);
        for (int n = 0; n < m->nfft; ++n) w[n] = (float)(0.5 - 0.5 * std::cos(2.0 * PI * n / m->nfft));
        TS_TRY(m->window.upload(w.data(), w.size() * sizeof(float)));
    }
    // ---- FFT twiddles, computed in double: the 1024-point complex passes and the real-transform split ----
    {
        if (m->nfft != 2048) return fail("ts_mfcc_create: the STFT kernel is built for n_fft = 2048");
        std::vector<float> a(2 * 1024), bq(2 * 1025);
        for (int i = 0; i < 1024; ++i) {
            a[2 * i] = (float)std::cos(2.0 * PI * i / 1024.0);
            a[2 * i + 1] = (float)(-std::sin(2.0 * PI * i / 1024.0));
        }
        for (int i = 0; i <= 1024; ++i) {
            bq[2 * i] = (float)std::cos(2.0 * PI * i / 2048.0);
            bq[2 * i + 1] = (float)(-std::sin(2.0 * PI * i / 2048.0));
        }
        TS_TRY(m->tw1024.upload(a.data(), a.size() * sizeof(float)));
        TS_TRY(m->tw2048.upload(bq.data(), bq.size() * sizeof(float)));
    }
    // ---- HTK mel filterbank (torchaudio.functional.melscale_fbanks, norm=None), transposed to [n_mels][n_freqs] ----
    {
        const int nb = m->nbins, nm = m->nmels;
        auto hz2mel = [](double f) { return 2595.0 * std::log10(1.0 + f / 700.0); };
        auto mel2hz = [](double x) { return 700.0 * (std::pow(10.0, x / 2595.0) - 1.0); };
        const double fmax = (double)(sr_out / 2);
        std::vector<double> fpts(nm + 2);
        const double m0 = hz2mel(0.0), m1 = hz2mel(fmax);
        for (int i = 0; i < nm + 2; ++i) fpts[i] = mel2hz(m0 + (m1 - m0) * i / (nm + 1));
        std::vector<float> fb((size_t)nm * m->nbins_pad, 0.f);
        for (int f = 0; f < nb; ++f) {
            const double freq = (double)(sr_out / 2) * f / (nb - 1);
            for (int j = 0; j < nm; ++j) {
                const double down = (freq - fpts[j]) / (fpts[j + 1] - fpts[j]);
                const double up = (fpts[j + 2] - freq) / (fpts[j + 2] - fpts[j + 1]);
                const double v = std::max(0.0, std::min(down, up));
                fb[(size_t)j * m->nbins_pad + f] = (float)v;
            }
        }
        TS_TRY(pack_linear_layer(fb.data(), m->nbins_pad, nullptr, nm, m->nbins_pad, &m->mel));
    }
    // ---- orthonormal DCT-II (torchaudio.functional.create_dct), [n_mfcc][n_mels] ----
    {
        const int nm = m->nmels, nc = m->nmfcc;
        std::vector<float> d((size_t)nc * nm);
        for (int k = 0; k < nc; ++k)
            for (int n = 0; n < nm; ++n) {
                double v = std::cos(PI / nm * (n + 0.5) * k);
                if (k == 0) v *= 1.0 / std::sqrt(2.0);
                d[(size_t)k * nm + n] = (float)(v * std::sqrt(2.0 / nm));
            }
        TS_TRY(pack_linear_layer(d.data(), nm, nullptr, nc, nm, &m->dct));
    }
    *out = m.release();
    return 0;
}
void ts_mfcc_destroy(ts_mfcc *m) { delete m; }

// stage 1 of ts_mfcc_forward on its own (get_mfcc_sepa resamples the whole clip first, then takes the MFCC of two parts):
// wav_dev (B,N) at sr_in -> out_dev (B, ts_mfcc_resampled_len(m, N)) at sr_out
long ts_mfcc_resampled_len(const ts_mfcc *m, long N) { return m ? m->resampled_len(N) : -1; }
int ts_mfcc_resample(ts_mfcc *m, const float *wav, int B, long N, float *out, void *stream) {
    if (!m || !wav || !out) return fail("ts_mfcc_resample: null argument");
    hipStream_t s = (hipStream_t)stream;
    MiscScope ms(m->ctx, s);
    if (m->sr_in == m->sr_out) {
        TS_HIP(hipMemcpyAsync(out, wav, (size_t)B * N * sizeof(float), hipMemcpyDeviceToDevice, s));
        return 0;
    }
    TS_HIP(launch_resample_polyphase(wav, B, (int)N, m->rs_kern.f(), m->norig, m->nnew, m->width, m->kw, out,
                                     (int)m->resampled_len(N), s));
    return 0;
}

// ---- librosa.load(sr=16000)'s resampler (face path, data_utils/utils.py:194): resampy 'kaiser_best' ---------------------
namespace {
struct KaiserTable {
    DevBuf win, delta;
    int nwin = 0, num_table = 512;
};
// half of a sinc windowed by a Kaiser window: 64 zero crossings, 512 samples per crossing (resampy's published
// 'kaiser_best' design: rolloff 0.9475937167399596, beta 14.769656459379492)
int kaiser_table(int device, const KaiserTable **out) {
    static std::mutex mu;
    static std::map<int, std::unique_ptr<KaiserTable>> tabs;
    std::lock_guard<std::mutex> g(mu);
    auto &t = tabs[device];
    if (!t) {
        const int num_zeros = 64, precision = 9, num_bits = 1 << precision, n = num_bits * num_zeros;
        const double rolloff = 0.9475937167399596, beta = 14.769656459379492, PI = 3.14159265358979323846;
        auto i0 = [](double x) {   // modified Bessel function of the first kind, order 0 (power series)
            double sum = 1.0, term = 1.0;
            for (int k = 1; k < 500; ++k) {
                term *= (x / (2.0 * k)) * (x / (2.0 * k));
                sum += term;
                if (term < 1e-18 * sum) break;
            }
            return sum;
        };
        std::vector<float> win(n + 1), delta(n + 1, 0.f);
        const int Mw = 2 * n + 1;   // the full symmetric Kaiser window; its right half [n:] tapers the sinc
        for (int i = 0; i <= n; ++i) {
            const double tpos = (double)num_zeros * i / n;                  // np.linspace(0, num_zeros, n + 1)
            const double a = rolloff * tpos * PI;
            const double sinc = a == 0.0 ? 1.0 : std::sin(a) / a;
            const double m = (double)(n + i) - (Mw - 1) / 2.0;            // scipy.signal.kaiser(M, beta)[n + i]
            const double r = 2.0 * m / (Mw - 1);
            const double taper = i0(beta * std::sqrt(std::max(0.0, 1.0 - r * r))) / i0(beta);
            win[i] = (float)(taper * rolloff * sinc);
        }
        for (int i = 0; i < n; ++i) delta[i] = win[i + 1] - win[i];
        std::unique_ptr<KaiserTable> k(new KaiserTable());
        k->nwin = n + 1;
        k->num_table = num_bits;
        TS_TRY(k->win.upload(win.data(), win.size() * sizeof(float)));
        TS_TRY(k->delta.upload(delta.data(), delta.size() * sizeof(float)));
        t = std::move(k);
    }
    *out = t.get();
    return 0;
}
}  // namespace

// output length of librosa.resample(fix=True): ceil(N * sr_out / sr_in); resampy itself produces int(N * ratio) samples and
// librosa.util.fix_length pads the (at most one) missing sample with zero
long ts_resample_kaiser_len(long N, int sr_in, int sr_out) {
    if (N < 0 || sr_in < 1 || sr_out < 1) return -1;
    return (long)std::ceil((double)N * (double)sr_out / (double)sr_in);
}
int ts_resample_kaiser(ts_ctx *ctx, const float *wav, int B, long N, int sr_in, int sr_out, float *out, void *stream) {
    if (!ctx || !wav || !out) return fail("ts_resample_kaiser: null argument");
    if (B < 1 || N < 1 || sr_in < 1 || sr_out < 1) return fail("ts_resample_kaiser: bad shape");
    hipStream_t s = (hipStream_t)stream;
    const long Nfix = ts_resample_kaiser_len(N, sr_in, sr_out);
    MiscScope ms(ctx, s);
    if (sr_in == sr_out) {
        TS_HIP(hipMemcpyAsync(out, wav, (size_t)B * N * sizeof(float), hipMemcpyDeviceToDevice, s));
        return 0;
    }
    const KaiserTable *kt = nullptr;
    TS_TRY(kaiser_table(ctx->device, &kt));
    const double ratio = (double)sr_out / (double)sr_in;
    const long Nres = (long)((double)N * ratio);          // int(shape * sample_ratio)
    if (Nres < 1) return fail("ts_resample_kaiser: input too short for this rate change");
    if (Nres < Nfix) TS_HIP(hipMemsetAsync(out, 0, (size_t)B * Nfix * sizeof(float), s));
    // rows of Nfix samples; the (at most one) sample beyond Nres stays zero (fix_length)
    const hipError_t e = launch_resample_kaiser(wav, B, (int)N, kt->win.f(), kt->delta.f(), kt->nwin, kt->num_table, ratio, out,
                                                (int)Nres, (int)Nfix, s);
    TS_HIP(e);
    return 0;
}

// number of MFCC frames for N input samples: T = floor(N_resampled / hop) + 1 (center=True)
int ts_mfcc_num_frames(const ts_mfcc *m, long N) { return m ? (int)(m->resampled_len(N) / m->hop) + 1 : -1; }

}  // extern "C"

// ---- the stages of ts_mfcc_forward / ts_mfcc_forward_mixed after the resampler, one launch each on the handle's own tables: shared by the two
// entries and by the test aids at the end of this file (talkshow_hip_debug.h); the caller opens the MiscScope.  ns = the DEVICE table of sample counts at the input rate and
// frames = the DEVICE frame table of a mixed pass; null = the uniform kernels. ----
namespace {
const char *const SHORT_CLIP = "clip shorter than half an FFT window (reflect padding undefined)";

// x (B, N) at the output rate -> power (B T, nbins_pad): framing + window + 2048-point real FFT + |X|^2 in one kernel (mfcc.hip)
int stft_stage(ts_mfcc *m, const float *x, const int *ns, int B, int N, int T, float *power, hipStream_t s) {
    if (ns)
        TS_HIP(launch_stft_power_lens(x, B, N, T, ns, m->norig, m->nnew, m->hop, m->window.f(), m->tw1024.f(), m->tw2048.f(), power,
                                      m->nbins_pad, s));
    else
        TS_HIP(launch_stft_power(x, B, N, T, m->hop, m->window.f(), m->tw1024.f(), m->tw2048.f(), power, m->nbins_pad, s));
    return 0;
}
// the mel projection (layer = m->mel) and the DCT (m->dct) on conv_gemm_f32: x (B T, ldx) -> out (B T, n); uniform passes run the rows as one
// clip of B T rows, mixed passes in the (B, T) row form with the length-masked epilogue (rows at or beyond frames[b]: +0.0)
int gemm_stage(ts_mfcc *m, const ConvLayer &layer, const float *x, int ldx, const int *frames, int B, int T, float *out, int n,
               hipStream_t s) {
    ConvParams p;
    if (frames) {
        conv_layer_params(layer, x, ldx, B, T, nullptr, 0, out, n, 0, n, &p);
        p.lens = frames;
    } else {
        conv_layer_params(layer, x, ldx, 1, B * T, nullptr, 0, out, n, 0, n, &p);
    }
    return run_conv(m->ctx, p, 0, s);
}
// mel (B, T nmels) in place: decibels and the per-clip clamp at (max - 80)
int db_stage(ts_mfcc *m, float *mel, const int *frames, int B, int T, hipStream_t s) {
    if (frames)
        TS_HIP(launch_db_topdb_lens(mel, B, T, m->nmels, frames, 80.0f, s));
    else
        TS_HIP(launch_db_topdb(mel, B, (long)T * m->nmels, 80.0f, s));
    return 0;
}
}  // namespace

extern "C" {

// wav_dev (B,N) mono fp32 at sr_in -> feat_dev (B,T,64), T = ts_mfcc_num_frames(m, N)
int ts_mfcc_forward(ts_mfcc *m, const float *wav, int B, long N, float *feat, void *stream) {
    if (!m || !wav || !feat) return fail("ts_mfcc_forward: null argument");
    hipStream_t s = (hipStream_t)stream;
    ts_ctx *ctx = m->ctx;
    const long N22 = m->resampled_len(N);
    if (N22 <= m->nfft / 2) return fail(std::string("ts_mfcc_forward: ") + SHORT_CLIP);
    const int T = (int)(N22 / m->hop) + 1;
    const long M = (long)B * T;
    ts_mfcc::Work &w = m->work(s);
    const size_t F = sizeof(float);
    const float *x22 = wav;
    {
        MiscScope ms(ctx, s);
        if (m->sr_in != m->sr_out) {
            TS_TRY(w.x22.ensure((size_t)B * N22 * F));
            TS_HIP(launch_resample_polyphase(wav, B, (int)N, m->rs_kern.f(), m->norig, m->nnew, m->width, m->kw, w.x22.f(), (int)N22, s));
            x22 = w.x22.f();
        }
        TS_TRY(w.power.ensure((size_t)M * m->nbins_pad * F));
        TS_TRY(stft_stage(m, x22, nullptr, B, (int)N22, T, w.power.f(), s));
    }
    TS_TRY(w.melb.ensure((size_t)M * m->nmels * F));
    TS_TRY(gemm_stage(m, m->mel, w.power.f(), m->nbins_pad, nullptr, B, T, w.melb.f(), m->nmels, s));
    {
        MiscScope ms(ctx, s);
        TS_TRY(db_stage(m, w.melb.f(), nullptr, B, T, s));
    }
    TS_TRY(gemm_stage(m, m->dct, w.melb.f(), m->nmels, nullptr, B, T, feat, m->nmfcc, s));
    return 0;
}

// ---- mixed passes: recordings of different lengths in one call (talkshow_hip.h) ---------------------------------------------------------
namespace {
// the host table of a mixed entry, checked before anything is launched: 1 <= ns[b] <= N_max
int check_counts(const char *who, const int32_t *ns_host, const int32_t *ns_dev, int B, long N_max) {
    if (!ns_host || !ns_dev) return fail(std::string(who) + ": null length table");
    if (B < 1 || N_max < 1 || N_max > 0x7fffffffl) return fail(std::string(who) + ": bad shape");
    for (int b = 0; b < B; ++b) {
        if (ns_host[b] < 1) return fail(std::string(who) + ": clip " + std::to_string(b) + " has no samples");
        if (ns_host[b] > N_max) return fail(std::string(who) + ": clip " + std::to_string(b) + " is longer than N_max");
    }
    return 0;
}
}  // namespace

int ts_mfcc_resample_mixed(ts_mfcc *m, const float *wav, const int32_t *ns_host, const int32_t *ns_dev, int B, long N_max, float *out,
                           void *stream) {
    if (!m || !wav || !out) return fail("ts_mfcc_resample_mixed: null argument");
    TS_TRY(check_counts("ts_mfcc_resample_mixed", ns_host, ns_dev, B, N_max));
    if (m->resampled_len(N_max) > 0x7fffffffl) return fail("ts_mfcc_resample_mixed: bad shape");
    hipStream_t s = (hipStream_t)stream;
    MiscScope ms(m->ctx, s);
    if (m->sr_in == m->sr_out) {
        TS_HIP(launch_copy_samples_lens(wav, B, (int)N_max, ns_dev, out, s));
        return 0;
    }
    TS_HIP(launch_resample_polyphase_lens(wav, B, (int)N_max, ns_dev, m->rs_kern.f(), m->norig, m->nnew, m->width, m->kw, out,
                                          (int)m->resampled_len(N_max), s));
    return 0;
}

int ts_resample_kaiser_mixed(ts_ctx *ctx, const float *wav, const int32_t *ns_host, const int32_t *ns_dev, int B, long N_max, int sr_in,
                             int sr_out, float *out, void *stream) {
    if (!ctx || !wav || !out) return fail("ts_resample_kaiser_mixed: null argument");
    if (sr_in < 1 || sr_out < 1) return fail("ts_resample_kaiser_mixed: bad shape");
    TS_TRY(check_counts("ts_resample_kaiser_mixed", ns_host, ns_dev, B, N_max));
    const long Nfix = ts_resample_kaiser_len(N_max, sr_in, sr_out);
    if (Nfix > 0x7fffffffl) return fail("ts_resample_kaiser_mixed: bad shape");
    hipStream_t s = (hipStream_t)stream;
    const double ratio = (double)sr_out / (double)sr_in;
    if (sr_in != sr_out)
        for (int b = 0; b < B; ++b)
            if ((long)((double)ns_host[b] * ratio) < 1)
                return fail("ts_resample_kaiser_mixed: clip " + std::to_string(b) + " is too short for this rate change");
    MiscScope ms(ctx, s);
    if (sr_in == sr_out) {
        TS_HIP(launch_copy_samples_lens(wav, B, (int)N_max, ns_dev, out, s));
        return 0;
    }
    const KaiserTable *kt = nullptr;
    TS_TRY(kaiser_table(ctx->device, &kt));
    TS_HIP(launch_resample_kaiser_lens(wav, B, (int)N_max, ns_dev, kt->win.f(), kt->delta.f(), kt->nwin, kt->num_table, ratio, out, (int)Nfix, s));
    return 0;
}

// The launch plan of ts_mfcc_forward on the padded block: the length variants of the three kernels that look across a recording's samples or
// rows, and the two GEMMs in the (B, T_max) row form with the length-masked epilogue (whole-tile plans only: sk_ok stays 0, so a row's bits do
// not depend on the rows it shares a launch with)
namespace {
// the front of both entries below, up to the mel projection: the checks under the entry's name, the workspace, then frames, resample, STFT and
// mel GEMM.  Returns the stream's workspace with melb (B, T, nmels: mel power, rows at or beyond a recording's own frames 0) and frames (B) filled
int mixed_mel(const char *who, ts_mfcc *m, const float *wav, const int32_t *ns_host, const int32_t *ns_dev, int B, long N_max, hipStream_t s,
              ts_mfcc::Work **w_out, int *T_out) {
    TS_TRY(check_counts(who, ns_host, ns_dev, B, N_max));
    const long N22 = m->resampled_len(N_max);
    const long T = N22 / m->hop + 1, M = (long)B * T;
    if (N22 > 0x7fffffffl || M > 0x7fffffffl) return fail(std::string(who) + ": bad shape");
    for (int b = 0; b < B; ++b)
        if (m->resampled_len(ns_host[b]) <= m->nfft / 2)
            return fail(std::string(who) + ": clip " + std::to_string(b) + " is shorter than half an FFT window (reflect padding undefined)");
    ts_mfcc::Work &w = m->work(s);
    const size_t F = sizeof(float);
    const float *x22 = wav;
    if (m->sr_in != m->sr_out) TS_TRY(w.x22.ensure((size_t)B * N22 * F));
    TS_TRY(w.power.ensure((size_t)M * m->nbins_pad * F));
    TS_TRY(w.melb.ensure((size_t)M * m->nmels * F));
    TS_TRY(w.frames.ensure((size_t)B * sizeof(int)));
    {
        MiscScope ms(m->ctx, s);
        TS_HIP(launch_mfcc_frames(ns_dev, B, (int)N_max, m->norig, m->nnew, m->hop, w.frames.i(), s));
        if (m->sr_in != m->sr_out) {
            TS_HIP(launch_resample_polyphase_lens(wav, B, (int)N_max, ns_dev, m->rs_kern.f(), m->norig, m->nnew, m->width, m->kw, w.x22.f(),
                                                  (int)N22, s));
            x22 = w.x22.f();
        }
        TS_TRY(stft_stage(m, x22, ns_dev, B, (int)N22, (int)T, w.power.f(), s));
    }
    *w_out = &w;
    *T_out = (int)T;
    return gemm_stage(m, m->mel, w.power.f(), m->nbins_pad, w.frames.i(), B, (int)T, w.melb.f(), m->nmels, s);
}
}  // namespace

int ts_mfcc_forward_mixed(ts_mfcc *m, const float *wav, const int32_t *ns_host, const int32_t *ns_dev, int B, long N_max, float *feat,
                          void *stream) {
    if (!m || !wav || !feat) return fail("ts_mfcc_forward_mixed: null argument");
    hipStream_t s = (hipStream_t)stream;
    ts_mfcc::Work *w = nullptr;
    int T = 0;
    TS_TRY(mixed_mel("ts_mfcc_forward_mixed", m, wav, ns_host, ns_dev, B, N_max, s, &w, &T));
    {
        MiscScope ms(m->ctx, s);
        TS_TRY(db_stage(m, w->melb.f(), w->frames.i(), B, T, s));
    }
    TS_TRY(gemm_stage(m, m->dct, w->melb.f(), m->nmels, w->frames.i(), B, T, feat, m->nmfcc, s));
    return 0;
}

// The maximum ts_mfcc_forward_mixed clamps each recording at: the same launches up to the mel projection, then the maximum of the dB
// expression over the recording's own rows.  out_dev (B,) fp32; nothing synchronises.
int ts_mfcc_peak_db_mixed(ts_mfcc *m, const float *wav, const int32_t *ns_host, const int32_t *ns_dev, int B, long N_max, float *out,
                          void *stream) {
    if (!m || !wav || !out) return fail("ts_mfcc_peak_db_mixed: null argument");
    hipStream_t s = (hipStream_t)stream;
    ts_mfcc::Work *w = nullptr;
    int T = 0;
    TS_TRY(mixed_mel("ts_mfcc_peak_db_mixed", m, wav, ns_host, ns_dev, B, N_max, s, &w, &T));
    MiscScope ms(m->ctx, s);
    TS_HIP(launch_db_peak_lens(w->melb.f(), B, T, m->nmels, w->frames.i(), out, s));
    return 0;
}

}  // extern "C"

// ---- wav sessions: the front end fed samples in chunks (talkshow_hip.h, "wav sessions") ---------------------------------------------------
// Host arithmetic of a session, from the rates alone (ts_mfcc_stream_plan needs no handle): after n samples, resampled outputs below
// final22(n) have every tap below n; frames below final_frames(n) have every sample — the reflected ones of the first rows included — below final22(n).
namespace {
struct WavClock {
    int norig = 1, nnew = 1, width = 0, kw = 0, hop = 734;
    long final22(long n) const { return n >= width ? (n - width) / norig * nnew : 0; }   // (j / nnew) norig - width + kw - 1 < n
    long total22(long n) const { return (nnew * n + norig - 1) / norig; }
    // row t reads resampled samples up to t hop + 1023, and row 0 — whose first sample, -1024, reflects to 1024 — one further
    static long frames_of(long j22, int hop) { return j22 >= 1025 ? (j22 - 1024) / hop + 1 : 0; }
    long final_frames(long n) const { return frames_of(final22(n), hop); }
    long flush_frames(long n) const { return total22(n) / hop + 1; }
    long in_keep0(long n) const { return std::max(0l, final22(n) / nnew * norig - width); }   // first input sample the next output reads
    static long x22_keep0(long frames, int hop) { return std::max(0l, frames * hop - 1025); }  // first resampled sample a later frame reads
};
int wav_clock(int sr_in, int sr_out, int fps, WavClock *c) {
    if (sr_in < 1 || sr_out < 1 || (fps != 30 && fps != 15)) return 1;
    c->hop = fps == 30 ? 734 : 1467;
    if (sr_in == sr_out) return 0;
    const int g = gcd_i(sr_in, sr_out);
    c->norig = sr_in / g;
    c->nnew = sr_out / g;
    c->width = (int)std::ceil(6.0 * c->norig / (std::min(c->norig, c->nnew) * 0.99));
    c->kw = 2 * c->width + c->norig;
    return 0;
}
}  // namespace

struct ts_mfcc_stream {
    ts_mfcc *m = nullptr;
    WavClock c;
    int B = 0, running = 1;
    long max_samples = 0, cap_in = 0, cap22 = 0, max_frames = 0;
    DevBuf in[2], x22[2], run_max, peak, power, melb;
    int cur_in = 0, cur22 = 0;
    long n_in = 0, in0 = 0;          // samples received; the sample at element 0 of in[cur_in]
    long j22 = 0, r0 = 0;            // resampled samples final; the resampled sample at element 0 of x22[cur22]
    long frames_out = 0;
    bool flushed = false;
    // test aid (ts_debug_mfcc_stream_tap): where every call also leaves its new resampled samples / power rows, by absolute index
    float *tap22 = nullptr, *tap_pw = nullptr;
    long tap22_ld = 0, tap_pw_rows = 0;
    size_t bytes() const {
        return in[0].bytes + in[1].bytes + x22[0].bytes + x22[1].bytes + run_max.bytes + peak.bytes + power.bytes + melb.bytes;
    }
};

namespace {
// one call of a session: the n new samples (flush: none, and the recording ends at the samples received)
int stream_call(ts_mfcc_stream *h, const float *wav, long n, bool flush, float *feat, int *frames, hipStream_t s) {
    ts_mfcc *m = h->m;
    ts_ctx *ctx = m->ctx;
    const WavClock &c = h->c;
    const int B = h->B;
    const long n1 = h->n_in + n;
    const long j1 = flush ? c.total22(n1) : c.final22(n1);
    const long t1 = flush ? c.flush_frames(n1) : c.final_frames(n1);
    const long F = t1 - h->frames_out;
    if (F < 0 || F > h->max_frames || j1 - h->r0 > h->cap22 || n1 - h->in0 > h->cap_in)
        return fail("ts_mfcc_stream: internal: a call outgrew the session's buffers");
    if (F > 0 && !feat) return fail("ts_mfcc_stream: null output");
    if (h->tap22 && j1 > h->tap22_ld) return fail("ts_debug_mfcc_stream_tap: the resampled samples outgrew the tap");
    if (h->tap_pw && t1 > h->tap_pw_rows) return fail("ts_debug_mfcc_stream_tap: the frames outgrew the tap");
    const bool same_rate = m->sr_in == m->sr_out;
    float *x22 = h->x22[h->cur22].f();
    {
        MiscScope ms(ctx, s);
        if (same_rate) {   // the resampler is a copy: the new samples are the new resampled samples
            TS_HIP(launch_stream_rows_copy(wav, n, 0, (int)n, x22 + (h->j22 - h->r0), h->cap22, B, s));
        } else {
            float *in = h->in[h->cur_in].f();
            TS_HIP(launch_stream_rows_copy(wav, n, 0, (int)n, in + (h->n_in - h->in0), h->cap_in, B, s));
            TS_HIP(launch_resample_polyphase_stream(in, h->cap_in, h->in0, n1, B, m->rs_kern.f(), c.norig, c.nnew, c.width, c.kw, x22, h->cap22,
                                                    h->r0, h->j22, j1, s));
        }
        if (h->tap22 && j1 > h->j22) {
            TS_HIP(launch_stream_rows_copy(x22, h->cap22, h->j22 - h->r0, (int)(j1 - h->j22), h->tap22 + h->j22, h->tap22_ld, B, s));
        }
        TS_HIP(launch_stft_power_stream(x22, h->cap22, h->r0, j1, B, (int)F, (int)h->frames_out, c.hop, m->window.f(), m->tw1024.f(),
                                        m->tw2048.f(), h->power.f(), m->nbins_pad, s));
        if (h->tap_pw && F > 0) {
            for (int b = 0; b < B; ++b)   // row b F + f -> row b tap_rows + frames_out + f
                TS_HIP(launch_stream_rows_copy(h->power.f() + (size_t)b * F * m->nbins_pad, 0, 0, (int)(F * m->nbins_pad),
                                               h->tap_pw + ((size_t)b * h->tap_pw_rows + h->frames_out) * m->nbins_pad, 0, 1, s));
        }
    }
    if (F > 0) {
        TS_TRY(gemm_stage(m, m->mel, h->power.f(), m->nbins_pad, nullptr, B, (int)F, h->melb.f(), m->nmels, s));
        {
            MiscScope ms(ctx, s);
            TS_HIP(launch_db_stream(h->melb.f(), B, (int)F, h->running ? nullptr : h->peak.f(), h->run_max.f(), 80.0f, s));
        }
        TS_TRY(gemm_stage(m, m->dct, h->melb.f(), m->nmels, nullptr, B, (int)F, feat, m->nmfcc, s));
    }
    if (!flush) {   // what later calls still read moves to the front of the twin buffers
        MiscScope ms(ctx, s);
        const long in0 = same_rate ? n1 : c.in_keep0(n1), r0 = WavClock::x22_keep0(t1, c.hop);
        if (!same_rate && in0 != h->in0) {
            TS_HIP(launch_stream_rows_copy(h->in[h->cur_in].f(), h->cap_in, in0 - h->in0, (int)(n1 - in0), h->in[h->cur_in ^ 1].f(), h->cap_in,
                                           B, s));
            h->cur_in ^= 1;
        }
        if (r0 != h->r0) {
            TS_HIP(launch_stream_rows_copy(x22, h->cap22, r0 - h->r0, (int)(j1 - r0), h->x22[h->cur22 ^ 1].f(), h->cap22, B, s));
            h->cur22 ^= 1;
        }
        h->in0 = in0;
        h->r0 = r0;
    }
    h->n_in = n1;
    h->j22 = j1;
    h->frames_out = t1;
    h->flushed = flush;
    if (frames) *frames = (int)F;
    return 0;
}
}  // namespace

extern "C" {

int ts_mfcc_stream_plan(int sr_in, int sr_out, int fps, long samples_before, long n, int flush, long *frames_before, long *frames_after) {
    WavClock c;
    if (wav_clock(sr_in, sr_out, fps, &c)) return fail("ts_mfcc_stream_plan: rates are positive and fps is 15 or 30");
    if (samples_before < 0 || n < 0) return fail("ts_mfcc_stream_plan: negative sample count");
    const long n1 = samples_before + n;
    if (flush && c.total22(n1) <= 1024) return fail(std::string("ts_mfcc_stream_plan: ") + SHORT_CLIP);
    if (frames_before) *frames_before = c.final_frames(samples_before);
    if (frames_after) *frames_after = flush ? c.flush_frames(n1) : c.final_frames(n1);
    return 0;
}

int ts_mfcc_stream_open(ts_mfcc *m, int B, long max_samples, int db_mode, const float *peak_db_dev, ts_mfcc_stream **out) {
    if (!m || !out) return fail("ts_mfcc_stream_open: null argument");
    if (B < 1 || max_samples < 1 || max_samples > (1l << 28)) return fail("ts_mfcc_stream_open: B and max_samples are at least 1 (max_samples at most 2^28)");
    if (db_mode != TS_WAV_DB_RUNNING && db_mode != TS_WAV_DB_PEAK) return fail("ts_mfcc_stream_open: db_mode is TS_WAV_DB_RUNNING or TS_WAV_DB_PEAK");
    if (db_mode == TS_WAV_DB_PEAK && !peak_db_dev) return fail("ts_mfcc_stream_open: TS_WAV_DB_PEAK needs the (B,) table of maxima");
    if (m->nmels != 256) return fail("ts_mfcc_stream_open: the session's dB kernel is built for 256 mel bands");
    TS_HIP(hipSetDevice(m->ctx->device));
    std::unique_ptr<ts_mfcc_stream> h(new ts_mfcc_stream());
    h->m = m;
    h->B = B;
    h->max_samples = max_samples;
    h->running = db_mode == TS_WAV_DB_RUNNING;
    WavClock &c = h->c;
    c.norig = m->norig; c.nnew = m->nnew; c.width = m->width; c.kw = m->kw; c.hop = m->hop;
    // new resampled samples of one call: a push finalises at most max_samples / norig + 1 more windows, the flush the width / norig + 2 held back
    const long new22 = std::max((max_samples / c.norig + 1) * c.nnew, ((long)c.width / c.norig + 2) * c.nnew + 1);
    h->cap_in = c.kw + max_samples;            // a tail of fewer than kw samples, then the call's own
    h->cap22 = 2049 + new22;                   // a tail of at most 2048 resampled samples, then the call's own
    h->max_frames = (2049 + new22) / c.hop + 2;
    const size_t F = sizeof(float);
    if (m->sr_in != m->sr_out)
        for (int i = 0; i < 2; ++i) TS_TRY(h->in[i].ensure((size_t)B * h->cap_in * F));
    for (int i = 0; i < 2; ++i) TS_TRY(h->x22[i].ensure((size_t)B * h->cap22 * F));
    TS_TRY(h->power.ensure((size_t)B * h->max_frames * m->nbins_pad * F));
    TS_TRY(h->melb.ensure((size_t)B * h->max_frames * m->nmels * F));
    std::vector<float> ninf((size_t)B, -INFINITY);
    TS_TRY(h->run_max.upload(ninf.data(), (size_t)B * F));
    if (!h->running) {
        TS_TRY(h->peak.ensure((size_t)B * F));
        TS_HIP(copy_and_wait(h->peak.p, peak_db_dev, (size_t)B * F, hipMemcpyDeviceToDevice));
    }
    *out = h.release();
    return 0;
}

int ts_mfcc_stream_push(ts_mfcc_stream *h, const float *wav, long n, float *feat, int *frames, void *stream) {
    if (!h || !frames) return fail("ts_mfcc_stream_push: null argument");
    if (h->flushed) return fail("ts_mfcc_stream_push: the session has been flushed (the recording has ended): open another");
    if (n < 0 || n > h->max_samples)
        return fail("ts_mfcc_stream_push: a push holds 0 to max_samples = " + std::to_string(h->max_samples) + " samples, got " + std::to_string(n));
    if (n > 0 && !wav) return fail("ts_mfcc_stream_push: null samples");
    if (h->n_in + n > (1l << 40)) return fail("ts_mfcc_stream_push: the session has run out of sample indices");
    return stream_call(h, wav, n, false, feat, frames, (hipStream_t)stream);
}

int ts_mfcc_stream_flush(ts_mfcc_stream *h, float *feat, int *frames, void *stream) {
    if (!h || !frames) return fail("ts_mfcc_stream_flush: null argument");
    if (h->flushed) return fail("ts_mfcc_stream_flush: the session has been flushed already");
    if (h->c.total22(h->n_in) <= h->m->nfft / 2) return fail(std::string("ts_mfcc_stream_flush: ") + SHORT_CLIP);
    return stream_call(h, nullptr, 0, true, feat, frames, (hipStream_t)stream);
}

long ts_mfcc_stream_samples_in(const ts_mfcc_stream *h) { return h ? h->n_in : -1; }
long ts_mfcc_stream_frames_out(const ts_mfcc_stream *h) { return h ? h->frames_out : -1; }
long ts_mfcc_stream_state_bytes(const ts_mfcc_stream *h) { return h ? (long)h->bytes() : -1; }
long ts_mfcc_stream_max_frames(const ts_mfcc_stream *h) { return h ? h->max_frames : -1; }
void ts_mfcc_stream_close(ts_mfcc_stream *h) { delete h; }
// the handle's resampler constants (norig, nnew, width, kw, hop): what the latency of a wav session is quoted from
void ts_mfcc_constants(const ts_mfcc *m, int32_t out[5]) {
    if (!m || !out) return;
    out[0] = m->norig; out[1] = m->nnew; out[2] = m->width; out[3] = m->kw; out[4] = m->hop;
}

// test aids: every later call of the session also leaves its new resampled samples in x22_dev (B rows of x22_ld, by absolute index) and its
// new power rows in power_dev (B, power_rows, nbins_pad), by frame index; null = off
int ts_debug_mfcc_stream_tap(ts_mfcc_stream *h, float *x22_dev, long x22_ld, float *power_dev, long power_rows) {
    if (!h) return fail("ts_debug_mfcc_stream_tap: null session");
    h->tap22 = x22_dev; h->tap22_ld = x22_ld; h->tap_pw = power_dev; h->tap_pw_rows = power_rows;
    return 0;
}
// the session's retained tails, in samples: input, resampled
void ts_debug_mfcc_stream_tails(const ts_mfcc_stream *h, long out[2]) {
    if (!h || !out) return;
    out[0] = h->n_in - h->in0; out[1] = h->j22 - h->r0;
}
// the session's dB kernel on caller-owned buffers: mel (B, F, 256) in place; peak (B,) or null = the running mode on run_max (B,)
int ts_debug_mfcc_stream_db(ts_mfcc *m, float *mel, int B, int F, const float *peak, float *run_max, void *stream) {
    if (!m || !mel || B < 1 || F < 1 || (!peak && !run_max)) return fail("ts_debug_mfcc_stream_db: bad argument");
    MiscScope ms(m->ctx, (hipStream_t)stream);
    TS_HIP(launch_db_stream(mel, B, F, peak, run_max, 80.0f, (hipStream_t)stream));
    return 0;
}

// ---- test aids (talkshow_hip_debug.h): the stages above on caller-owned device buffers; nothing is allocated, `stream` is not synchronized ----
int ts_debug_mfcc_stft(ts_mfcc *m, const float *x, int B, long N, float *power, void *stream) {
    if (!m || !x || !power || B < 1 || N < 1 || N > 0x7fffffffl) return fail("ts_debug_mfcc_stft: bad argument");
    if (N <= m->nfft / 2) return fail(std::string("ts_debug_mfcc_stft: ") + SHORT_CLIP);
    const long T = N / m->hop + 1;
    if ((long)B * T > 0x7fffffffl) return fail("ts_debug_mfcc_stft: bad shape");
    MiscScope ms(m->ctx, (hipStream_t)stream);
    return stft_stage(m, x, nullptr, B, (int)N, (int)T, power, (hipStream_t)stream);
}
int ts_debug_mfcc_stft_lens(ts_mfcc *m, const float *x, const int32_t *ns_host, const int32_t *ns_dev, int B, long N, float *power,
                            void *stream) {
    if (!m || !x || !power || !ns_host || !ns_dev || B < 1 || N < 1 || N > 0x7fffffffl) return fail("ts_debug_mfcc_stft_lens: bad argument");
    for (int b = 0; b < B; ++b) {
        const long nb = ns_host[b] < 1 ? 0 : m->resampled_len(ns_host[b]);
        if (nb > N) return fail("ts_debug_mfcc_stft_lens: clip " + std::to_string(b) + " is longer than the rows");
        if (nb <= m->nfft / 2) return fail("ts_debug_mfcc_stft_lens: clip " + std::to_string(b) + ": " + SHORT_CLIP);
    }
    const long T = N / m->hop + 1;
    if ((long)B * T > 0x7fffffffl) return fail("ts_debug_mfcc_stft_lens: bad shape");
    MiscScope ms(m->ctx, (hipStream_t)stream);
    return stft_stage(m, x, ns_dev, B, (int)N, (int)T, power, (hipStream_t)stream);
}
int ts_debug_mfcc_frames(ts_mfcc *m, const int32_t *ns_dev, int B, long N_max, int32_t *frames_dev, void *stream) {
    if (!m || !ns_dev || !frames_dev || B < 1 || N_max < 1 || N_max > 0x7fffffffl) return fail("ts_debug_mfcc_frames: bad argument");
    hipStream_t s = (hipStream_t)stream;
    MiscScope ms(m->ctx, s);
    TS_HIP(launch_mfcc_frames(ns_dev, B, (int)N_max, m->norig, m->nnew, m->hop, frames_dev, s));
    return 0;
}
int ts_debug_mfcc_mel(ts_mfcc *m, const float *power, const int32_t *frames_dev, int B, int T, float *mel, void *stream) {
    if (!m || !power || !mel || B < 1 || T < 1 || (long)B * T > 0x7fffffffl) return fail("ts_debug_mfcc_mel: bad argument");
    return gemm_stage(m, m->mel, power, m->nbins_pad, frames_dev, B, T, mel, m->nmels, (hipStream_t)stream);
}
int ts_debug_mfcc_db(ts_mfcc *m, float *mel, const int32_t *frames_dev, int B, int T, void *stream) {
    if (!m || !mel || B < 1 || T < 1) return fail("ts_debug_mfcc_db: bad argument");
    MiscScope ms(m->ctx, (hipStream_t)stream);
    return db_stage(m, mel, frames_dev, B, T, (hipStream_t)stream);
}
int ts_debug_mfcc_dct(ts_mfcc *m, const float *mel, const int32_t *frames_dev, int B, int T, float *feat, void *stream) {
    if (!m || !mel || !feat || B < 1 || T < 1 || (long)B * T > 0x7fffffffl) return fail("ts_debug_mfcc_dct: bad argument");
    return gemm_stage(m, m->dct, mel, m->nmels, frames_dev, B, T, feat, m->nmfcc, (hipStream_t)stream);
}

}  // extern "C"
