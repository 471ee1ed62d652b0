// afis_train.cpp — codebook training of the C ABI (include/afis_matcher.h has the definition): afis_pq_train (Lloyd steps on the device, pq_train.hip; the division
// of a step's integer sums by its counts here, in IEEE fp64), afis_pq_train_init_points (the reproducible minit='points' rule, pq_train_plan.h) and
// afis_codebook_write.  Replaces extraction/descriptor_PQ.py:64-77 (training: kmeans2 per sub-space).  No context: a context needs a codebook.  Host C++ only.
#include "afis_ctx.h"
#include "pq_train.h"
#include "pq_train_plan.h"

using namespace afis;

namespace {

constexpr size_t kCwFloats = (size_t)kM * kK * kDsub;          // 24 576
constexpr int64_t kSlicePoints = 1 << 18;                      // points per upload slice of the first pass: 96 MiB of staging

// The device state of one call; everything is allocated before anything is queued.
struct TrainDev {
    hipStream_t stream = nullptr;
    DevBuf xt, labels, stage, cw, acc, bad;
    unsigned long long* h_acc = nullptr;                       // pinned: a step's sums, counts and changed count; behind them the first pass's flag
    bool abandoned = false;                                    // a wait ran out: the device may still be working — its buffers are left alone
    ~TrainDev()
    {
        if (abandoned) return;
        xt.release(); labels.release(); stage.release(); cw.release(); acc.release(); bad.release();
        if (h_acc) (void)hipHostFree(h_acc);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

// Bounded host wait, as afis_search.cpp::wait_streams: hipStreamQuery until done or AFIS_SEARCH_TIMEOUT_S (default 600 s; <= 0: unbounded hipStreamSynchronize)
int train_wait(TrainDev& d, const char* what)
{
    double limit = 600.0;
    if (const char* r = getenv("AFIS_SEARCH_TIMEOUT_S")) limit = atof(r);
    if (limit <= 0) {
        const hipError_t e = hipStreamSynchronize(d.stream);
        return e == hipSuccess ? AFIS_OK : fail(nullptr, AFIS_EDEVICE, std::string(what) + ": hipStreamSynchronize: " + hipGetErrorString(e));
    }
    const auto t0 = std::chrono::steady_clock::now();
    for (long spins = 0;; ++spins) {
        const hipError_t e = hipStreamQuery(d.stream);
        if (e == hipSuccess) return AFIS_OK;
        if (e != hipErrorNotReady) return fail(nullptr, AFIS_EDEVICE, std::string(what) + ": hipStreamQuery: " + hipGetErrorString(e));
        if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > limit) {
            d.abandoned = true;
            char msg[200];
            snprintf(msg, sizeof msg, "%s: the device did not finish within %.3g s (AFIS_SEARCH_TIMEOUT_S)", what, limit);
            return fail(nullptr, AFIS_EDEVICE, msg);
        }
        if (spins < 20000) std::this_thread::yield(); else std::this_thread::sleep_for(std::chrono::microseconds(50));
    }
}

#define TRCHK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return fail(nullptr, AFIS_EDEVICE, std::string("afis_pq_train: " #call ": ") + hipGetErrorString(e_)); } while (0)

// The update of include/afis_matcher.h: one int64 -> fp64 conversion, one fp64 division by an exact divisor, one fp64 -> fp32 rounding; count 0 keeps the old bits.
void train_update(const unsigned long long* acc, float* cw)
{
    for (size_t c = 0; c < (size_t)kM * kK; ++c) {
        const int64_t count = (int64_t)acc[c * kTrainAcc + kDsub];
        if (count <= 0) continue;
        const double div = (double)count * 1073741824.0;
        for (int d = 0; d < kDsub; ++d) cw[c * kDsub + d] = (float)((double)(int64_t)acc[c * kTrainAcc + d] / div);
    }
}

}  // namespace

extern "C" {

int afis_pq_train(int device_id, const float* des, int64_t n, const float* init, int iters, float* codewords, int64_t* counts, int64_t* changed, int* iters_run)
{
    if (!init || !codewords || n < 0 || (n > 0 && !des)) return fail(nullptr, AFIS_EINVAL, "afis_pq_train: null argument or negative size");
    if (iters < 0 || iters > 1000) return fail(nullptr, AFIS_EINVAL, "afis_pq_train: iters must lie in 0 .. 1000");
    if (n > kTrainMaxPoints) return fail(nullptr, AFIS_EINVAL, "afis_pq_train: more than 2^26 points (the int64 sums are sized for |x| <= 64 and n <= 2^26)");
    for (size_t i = 0; i < kCwFloats; ++i)
        if (!std::isfinite(init[i])) return fail(nullptr, AFIS_EINVAL, "afis_pq_train: init holds a component that is not finite");
    std::vector<float> cur(init, init + kCwFloats);
    std::vector<int64_t> cnt((size_t)kM * kK, 0), chg((size_t)iters, 0);
    int run = 0;
    if (iters > 0 && n > 0) {
        int n_dev = 0;
        if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) return fail(nullptr, AFIS_EDEVICE, "afis_pq_train: no HIP device (this library has no CPU fallback)");
        if (device_id < 0 || device_id >= n_dev) return fail(nullptr, AFIS_EINVAL, "afis_pq_train: device_id out of range");
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, device_id) != hipSuccess) return fail(nullptr, AFIS_EDEVICE, "afis_pq_train: hipGetDeviceProperties failed");
        if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
            return fail(nullptr, AFIS_EDEVICE, std::string("afis_pq_train: kernels are built for gfx950 only, device is ") + prop.gcnArchName);
        TRCHK(hipSetDevice(device_id));
        TrainDev d;
        // every allocation before any device work: the resident points (384 n bytes), the labels (16 n), one upload slice, the codebook and the accumulators
        const int64_t slice = std::min<int64_t>(n, kSlicePoints);
        const size_t acc_bytes = (kTrainSumWords + 1) * sizeof(unsigned long long);
        TRCHK(hipStreamCreateWithFlags(&d.stream, hipStreamNonBlocking));
        TRCHK(d.xt.ensure((size_t)n * kDes * 4));
        TRCHK(d.labels.ensure((size_t)n * kM));
        TRCHK(d.stage.ensure((size_t)slice * kDes * 4));
        TRCHK(d.cw.ensure(kCwFloats * 4));
        TRCHK(d.acc.ensure(acc_bytes));
        TRCHK(d.bad.ensure(16));
        TRCHK(hipHostMalloc((void**)&d.h_acc, acc_bytes + 16, hipHostMallocDefault));
        uint32_t* h_bad = reinterpret_cast<uint32_t*>(d.h_acc + kTrainSumWords + 1);
        static const bool trace = getenv("AFIS_TRAIN_TRACE") != nullptr;    // development aid: the device time of the first pass and of every step, on stderr
        Events ev(2);
        for (hipEvent_t& e : ev) TRCHK(hipEventCreate(&e));

        // first pass: the points to the device slice by slice, transposed to [16][n][6] and validated
        TRCHK(hipMemsetAsync(d.bad.p, 0, 16, d.stream));
        TRCHK(hipEventRecord(ev[0], d.stream));
        for (int64_t p0 = 0; p0 < n; p0 += slice) {
            const int64_t np = std::min(slice, n - p0);
            TRCHK(hipMemcpyAsync(d.stage.p, des + p0 * kDes, (size_t)np * kDes * 4, hipMemcpyHostToDevice, d.stream));
            TRCHK(launch_train_transpose(d.stage.as<float>(), p0, np, n, d.xt.as<float>(), d.bad.as<uint32_t>(), d.stream));
        }
        TRCHK(hipEventRecord(ev[1], d.stream));
        TRCHK(hipMemcpyAsync(h_bad, d.bad.p, 4, hipMemcpyDeviceToHost, d.stream));
        AFISCHK(train_wait(d, "afis_pq_train: the first pass"));
        if (*h_bad) return fail(nullptr, AFIS_EINVAL, "afis_pq_train: des holds a component that is not finite or exceeds 64 in magnitude");
        if (trace) { float ms = 0; (void)hipEventElapsedTime(&ms, ev[0], ev[1]); fprintf(stderr, "afis_pq_train: first pass %.3f ms (uploads included)\n", ms); }

        for (int t = 0; t < iters; ++t) {
            TRCHK(hipMemcpyAsync(d.cw.p, cur.data(), kCwFloats * 4, hipMemcpyHostToDevice, d.stream));
            TRCHK(hipEventRecord(ev[0], d.stream));
            TRCHK(hipMemsetAsync(d.acc.p, 0, acc_bytes, d.stream));
            TRCHK(launch_train_step(d.xt.as<float>(), n, d.cw.as<float>(), d.labels.as<uint8_t>(), t == 0, d.acc.as<unsigned long long>(), d.stream));
            TRCHK(hipEventRecord(ev[1], d.stream));
            TRCHK(hipMemcpyAsync(d.h_acc, d.acc.p, acc_bytes, hipMemcpyDeviceToHost, d.stream));
            AFISCHK(train_wait(d, "afis_pq_train: a step"));
            train_update(d.h_acc, cur.data());
            for (size_t c = 0; c < (size_t)kM * kK; ++c) cnt[c] = (int64_t)d.h_acc[c * kTrainAcc + kDsub];
            chg[t] = (int64_t)d.h_acc[kTrainSumWords];
            run = t + 1;
            if (trace) { float ms = 0; (void)hipEventElapsedTime(&ms, ev[0], ev[1]); fprintf(stderr, "afis_pq_train: step %d device %.3f ms changed %lld\n", t, ms, (long long)chg[t]); }
            if (t >= 1 && chg[t] == 0) break;                    // a fixed point: the next step would repeat this one's labels, sums and codewords
        }
    }
    memcpy(codewords, cur.data(), kCwFloats * 4);
    if (counts) memcpy(counts, cnt.data(), cnt.size() * sizeof(int64_t));
    if (changed && iters > 0) memcpy(changed, chg.data(), chg.size() * sizeof(int64_t));
    if (iters_run) *iters_run = run;
    return AFIS_OK;
}

int afis_pq_train_init_points(const float* des, int64_t n, uint64_t seed, float* init)
{
    if (!des || !init) return fail(nullptr, AFIS_EINVAL, "afis_pq_train_init_points: null argument");
    if (n < kTrainInitK) return fail(nullptr, AFIS_EINVAL, "afis_pq_train_init_points: fewer than 256 points");
    int64_t idx[kTrainInitK];
    for (int m = 0; m < kM; ++m) {
        train_init_indices(n, seed, m, idx);
        for (int k = 0; k < kK; ++k) memcpy(init + ((size_t)m * kK + k) * kDsub, des + (size_t)idx[k] * kDes + m * kDsub, kDsub * sizeof(float));
    }
    return AFIS_OK;
}

int afis_codebook_write(const float* codewords, int M, int K, int dsub, void* out, size_t out_cap, size_t* out_len)
{
    if (!codewords || !out_len) return fail(nullptr, AFIS_EINVAL, "afis_codebook_write: null argument");
    if (M != kM || K != kK || dsub != kDsub) return fail(nullptr, AFIS_EINVAL, "afis_codebook_write: only the M=16, K=256, dsub=6 codebook geometry is supported");
    const int16_t head[3] = {(int16_t)M, (int16_t)K, (int16_t)dsub};
    *out_len = sizeof head + kCwFloats * 4;
    if (!out) return AFIS_OK;
    if (out_cap < *out_len) return fail(nullptr, AFIS_EINVAL, "afis_codebook_write: output buffer too small");
    memcpy(out, head, sizeof head);
    memcpy((uint8_t*)out + sizeof head, codewords, kCwFloats * 4);
    return AFIS_OK;
}

}  // extern "C"
