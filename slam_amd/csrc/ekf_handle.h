// The device EKF's handle (include/slamgpu.h: slamgpu_ekf), as its two units see it: ekf.cpp (the filter's kernels and entry points)
// and ekf_local.cpp (the local period: slamgpu_ekf_local_*).  Private, after slamgpu_ctx.h.
#pragma once
#include "slamgpu_ctx.h"
#include "ekf_helpers.h"

namespace {

constexpr int kTile = 128;   // tile of P per workgroup of ekf_syrk_kernel and of the commit's products
constexpr int kKStep = 32;   // k columns staged in LDS at a time; a chunk's K is padded with zeros to a multiple of it

}  // namespace

// (named at namespace scope, not private to a unit: functions of one unit that the other calls take and return them)
// the small device work area, by value.  flag: [0] the chunk's factorisation succeeded, [1] sticky status bits, [2] ekf_predict_kernel's ticket
struct EkfWork {
    float *H5;  // [kChunk][10]
    float *v;   // [kKMax] innovation
    float *t;   // [kKMax] U^-T v
    float *Ui;  // [kKMax][kKMax] inverse of the upper factor
    float *hv;  // [2] heading update: innovation, S
    float *c2;  // [ld] heading update: column 2 of P before it
    float *Wh;  // [ld] heading update: gain
    int32_t *flag;
};

// what a stage works on: the filter's own P and x, or the local period's extended matrix (ekf_local.cpp).  n: the extent the kernels
// cover, nf: the features the gates and idf may name, len: where augment appends
struct EkfMat {
    float *P, *x, *PHt, *W1;
    int ld, n, nf, len;
    EkfWork w;
};

// A local period ("local periods").  The extended matrix M, row stride ld: the active state at [0, 3 + 2 (k +
// n_new)), room for max_new features up to off, the na0 carried entries (phi's columns, -psi, theta in x) at [off, off + na0).  What
// lies between the active state and off is ZERO (the diagonal: the heading update's eps, h times) and stays so under every stage,
// so the filter's own kernels run on M over [0, off + na0) as they are.  psi is ALSO kept apart in float64 (psi, [na0][na0]), summed
// from the float32 factors of every chunk and heading update, and that copy is what the commit uses: entries of psi are thousands of
// times those of Y^T psi Y, and the float32 block of M loses the commit an order of magnitude of accuracy (profiles/ekf_local.txt)
struct EkfLocal {
    bool open = false;
    int k = 0, max_new = 0, n_new = 0, na0 = 0, off = 0, ld = 0, dim0 = 0, nB = 0, ldY = 0;
    int64_t calls = 0, commits = 0;
    std::vector<int32_t> feat;  // [k] the active features at begin, global, ascending
    std::vector<int32_t> g2l;   // [nf at begin] global feature -> local, -1 passive
    DevBuf<float> M, x, Y, PHt, W1, cw;
    DevBuf<double> psi, T;      // psi [na0][na0]; T = psi Y [na0][ldY], made by the commit
    DevBuf<int32_t> idx;        // gmap [off]: local state index -> global | bidx [nB]: passive -> global | cmap [dim0]: global -> local, or -(passive + 1)
    PinBuf<int32_t> idx_host;
    hipEvent_t idx_ev = nullptr;  // the device has taken idx_host
    bool idx_used = false;
    EkfWork w{};
    int dimA() const { return 3 + 2 * (k + n_new); }
};

// slamgpu_ekf_feature_stats: per-feature counts, host only.  An epoch is a successful sim with observations or a successful direct
// update; the call in progress counts hits and births at epoch + 1 and advances epoch when it has succeeded
struct EkfFeatureStats {
    int32_t epoch = 0;
    std::vector<int32_t> hits, born, last;
    void append(int n, int32_t at) {
        hits.insert(hits.end(), (size_t) n, 0);
        born.insert(born.end(), (size_t) n, at);
        last.insert(last.end(), (size_t) n, at);
    }
    void observed(const int32_t *idf, int32_t m, int32_t at) {  // global feature indices
        for (int32_t i = 0; i < m; i++) {
            hits[(size_t) idf[i]]++;
            last[(size_t) idf[i]] = at;
        }
    }
    void uploaded(int nf) {
        hits.assign((size_t) nf, 0);
        born.assign((size_t) nf, epoch);
        last.assign((size_t) nf, epoch);
    }
    void remove(const int32_t *features, int32_t k) {  // ascending and distinct
        size_t out = 0;
        int32_t q = 0;
        for (size_t f = 0; f < hits.size(); f++) {
            if (q < k && (size_t) features[q] == f) {
                q++;
                continue;
            }
            hits[out] = hits[f];
            born[out] = born[f];
            last[out] = last[f];
            out++;
        }
        hits.resize(out);
        born.resize(out);
        last.resize(out);
    }
};

struct slamgpu_ekf {
    slamgpu_ekf_config cfg{};
    EkfStream stream;
    int dim = 3, ld = 0, cap_dim = 0;  // dim: the full filter's, inside a local period too
    DevBuf<float> P, x, PHt, W1, work, z_dev, blk_dev;
    DevBuf<int32_t> flag, lab_dev, idx_dev;
    PinBuf<char> pin;
    EkfWork w{};
    EkfIdTable table;  // association_known
    EkfLocal loc;
    EkfFeatureStats stats;
    // slamgpu_ekf_remove: src [dim'] the surviving state indices, staged through rm_host
    DevBuf<int32_t> rm_src;
    PinBuf<int32_t> rm_host;
    hipEvent_t rm_ev = nullptr;  // the device has taken rm_host
    bool rm_used = false;
};

#pragma GCC visibility push(hidden)
// ekf.cpp's, as ekf_local.cpp calls it
int ekf_check(slamgpu_ekf *e);
// ekf_local.cpp's, as the stages of ekf.cpp call them while a period is open
EkfMat ekf_local_mat(slamgpu_ekf *e);
int ekf_local_features(slamgpu_ekf *e, const int32_t *idf, int32_t m, std::vector<int32_t> &local);  // global -> local; an inactive one: SLAMGPU_ERR_INVALID
void ekf_local_labels(slamgpu_ekf *e, int32_t *labels, int32_t nz);                                   // local -> global, in place
int ekf_local_augment_carried(slamgpu_ekf *e, float r, float b);  // the new feature's rows over the carried entries, before the augment kernel
int ekf_local_chunk(slamgpu_ekf *e, int n);   // psi += G1 G1^T of the chunk whose gain kernel has just been enqueued (n rows of innovation)
int ekf_local_heading(slamgpu_ekf *e);        // ... and of the heading update whose kernels have just been enqueued
void ekf_local_release(slamgpu_ekf *e);
#pragma GCC visibility pop
