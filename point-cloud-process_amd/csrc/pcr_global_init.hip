// Global initialisation in front of ICP (Registration/main.py:33-84, icp_template.py:20-41,56-110), host side: the calls that chain the
// stages of pcr_features.hip, pcr_match.hip and pcr_ransac.hip -- per scan and per pair (pcr_preprocess, pcr_global_registration) and
// for a whole share of pairs at once (pcr_global_init_batch).  No kernel lives here.
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <thread>
#include <vector>
#include "pcr_global_dev.h"

// preprocess_point_cloud's result (Registration/main.py:33-47), resident on the device: the down-sampled cloud (records in row
// order: id == position), its normals (n,3) and its FPFH descriptors (n,33)
struct pcr_prep {
    pcr_cloud* down = nullptr;
    double* normals = nullptr;
    double* fpfh = nullptr;
    int64_t n = 0;
};

extern "C" {

int pcr_prep_free(pcr_ctx* ctx, pcr_prep* p) {
    if (!p) return PCR_OK;
    if (!ctx) return PCR_E_INVALID;
    if (p->normals) pcr_dev_free(ctx, p->normals);
    if (p->fpfh) pcr_dev_free(ctx, p->fpfh);
    if (p->down) pcr_cloud_free(ctx, p->down);
    delete p;
    return PCR_OK;
}

int64_t pcr_prep_size(const pcr_prep* p) { return p ? p->n : 0; }
const pcr_cloud* pcr_prep_cloud(const pcr_prep* p) { return p ? p->down : nullptr; }

int pcr_preprocess(pcr_ctx* ctx, const pcr_cloud* cloud, double voxel_size, double normal_radius, int normal_max_nn, double fpfh_radius, int fpfh_max_nn,
                   pcr_prep** out) try {
    if (!ctx || !cloud || !out || !prep_params_ok(voxel_size, normal_radius, normal_max_nn, fpfh_radius, fpfh_max_nn)) return PCR_E_INVALID;
    *out = nullptr;
    if (cloud->n <= 0) return PCR_E_EMPTY;
    hipSetDevice(ctx->device);
    pcr_owned<pcr_prep, pcr_prep_free> p(ctx, new pcr_prep());
    int rc = pcr_voxel_filter_cloud(ctx, cloud, voxel_size, 2, 0, &p->down);   // mode 2 = Open3D's voxel_down_sample (main.py:35)
    if (rc == PCR_OK) {
        p->n = p->down->n;
        rc = pcr_dev_alloc(ctx, sizeof(double) * 3 * p->n, (void**)&p->normals);
    }
    if (rc == PCR_OK) rc = pcr_dev_alloc(ctx, sizeof(double) * 33 * p->n, (void**)&p->fpfh);
    if (rc == PCR_OK) rc = pcr_hybrid_normals_device(ctx, p->down, normal_radius, normal_max_nn, 1, nullptr, p->normals);
    if (rc == PCR_OK) rc = pcr_fpfh_device(ctx, p->down, p->normals, fpfh_radius, fpfh_max_nn, p->fpfh);
    if (rc == PCR_OK) rc = pcr_read_fail(ctx);
    if (rc != PCR_OK) { pcr_sync(ctx->stream); return rc; }
    *out = p.release();
    return PCR_OK;
} PCR_CATCH(ctx)

int pcr_prep_download(pcr_ctx* ctx, const pcr_prep* p, double* points, double* normals, double* features) {
    if (!ctx || !p) return PCR_E_INVALID;
    hipSetDevice(ctx->device);
    if (points) { const int rc = pcr_cloud_download_f64(ctx, p->down, points); if (rc) return rc; }
    if (normals) PCR_HIP(ctx, hipMemcpyAsync(normals, p->normals, sizeof(double) * 3 * p->n, hipMemcpyDeviceToHost, ctx->stream));
    if (features) PCR_HIP(ctx, hipMemcpyAsync(features, p->fpfh, sizeof(double) * 33 * p->n, hipMemcpyDeviceToHost, ctx->stream));
    PCR_HIP(ctx, pcr_sync(ctx->stream));
    return PCR_OK;
}

int pcr_global_registration(pcr_ctx* ctx, const pcr_prep* source, const pcr_prep* target, const pcr_ransac_params* prm, int mutual_filter,
                            pcr_ransac_result* res) {
    if (!ctx || !source || !target || !res || !ransac_params_ok(prm)) return PCR_E_INVALID;
    if (source->n <= 0 || target->n <= 0) return PCR_E_EMPTY;
    hipSetDevice(ctx->device);
    const long long na = source->n, nb = target->n;
    pcr_dev_block ij(ctx), ji(ctx), dab(ctx), dba(ctx), corr(ctx);
    int rc;
    if ((rc = ij.alloc(sizeof(int) * na)) || (rc = ji.alloc(sizeof(int) * nb)) || (rc = dab.alloc(sizeof(double) * na)) || (rc = dba.alloc(sizeof(double) * nb)) ||
        (rc = corr.alloc(sizeof(int) * 2 * na + 16)))
        return rc;
    if ((rc = pcr_feature_match_device(ctx, source->fpfh, na, target->fpfh, nb, 33, ij.as<int>(), dab.as<double>()))) return rc;
    if (mutual_filter && (rc = pcr_feature_match_device(ctx, target->fpfh, nb, source->fpfh, na, 33, ji.as<int>(), dba.as<double>()))) return rc;
    int* const d_m = corr.as<int>() + 2 * na;
    pcr_corr_build(ctx, ij.as<int>(), ji.as<int>(), (int)na, mutual_filter ? 1 : 0, corr.as<int>(), d_m);
    // the sampled records by ROW: the down-sampled clouds are written in row order, but a caller that has used one as the query
    // cloud of a search since (pcr_nn1 lays its queries out along the index's curve, in place) has re-ordered it
    const pcr_pt *s_rows = source->down->d, *t_rows = target->down->d;
    pcr_dev_block s_tmp(ctx), t_tmp(ctx);
    if (source->down->morton_sorted) {
        if ((rc = s_tmp.alloc(sizeof(pcr_pt) * na)) || (rc = pcr_cloud_rows(ctx, source->down, s_tmp.as<pcr_pt>()))) return rc;
        s_rows = s_tmp.as<pcr_pt>();
    }
    if (target->down->morton_sorted) {
        if ((rc = t_tmp.alloc(sizeof(pcr_pt) * nb)) || (rc = pcr_cloud_rows(ctx, target->down, t_tmp.as<pcr_pt>()))) return rc;
        t_rows = t_tmp.as<pcr_pt>();
    }
    return pcr_ransac_device(ctx, s_rows, t_rows, corr.as<int>(), d_m, prm, res);
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------ the pair loop's initialisation, fused
// prepare_dataset + execute_global_registration (Registration/main.py:197-203) for a whole share of pairs on ONE context: the scans
// are packed into pinned memory by a few host threads and copied once; ONE sort down-samples all of them (pcr_voxel_downsample_scans);
// normals, SPFH and FPFH are one launch each over every down-sampled point of the chunk (a block's search space is its own scan); matching,
// correspondence sets and the RANSAC loop run for all pairs side by side.  Same arithmetic, same order, same seeds as pcr_preprocess +
// pcr_global_registration pair by pair: the results are bit for bit those (tests/test_gpu_global_init.py).
// Returns PCR_E_UNSUPPORTED when the share does not fit this path (a down-sampled scan above HYBRID_BRUTE_MAX points, a neighbourhood
// that cannot be bounded, extents too large for the packed key): the caller then takes the scans one by one.
namespace {
constexpr int64_t CHUNK_PTS = 16ll << 20;
constexpr int CHUNK_SCANS = 2048, PAIR_CHUNK = 512;
// the scans of a chunk in the pinned block: ds[q] = scan who[q] (row of clouds[]), `at` points in all
struct chunk_plan { std::vector<pcr_down_scan> ds; std::vector<int64_t> who; unsigned int at = 0; };
// what stays of a chunk on the device until the last pair is done
struct scan_chunk {
    pcr_dev_block down, vsid, scan_first, fpfh;   // records, their scan, first record of every scan; FPFH (ng,33)
    // matrix-core operands of the descriptors (feature_match_mfma_jobs_kernel): per scan ceil(n / 16) tiles from tile_first[scan]
    pcr_dev_block op_t, op_q, norm2, max_norm2, min_row;
    int64_t ng = 0; int n_scans = 0;
    std::vector<unsigned int> first, tile_first;   // host copy of scan_first; first tile of every scan
    explicit scan_chunk(pcr_ctx* c) : down(c), vsid(c), scan_first(c), fpfh(c), op_t(c), op_q(c), norm2(c), max_norm2(c), min_row(c) {}
    // (the order in which blocks go back decides which addresses later allocations get: this one, chunk by chunk)
    ~scan_chunk() { for (pcr_dev_block* b : {&down, &vsid, &scan_first, &fpfh, &op_t, &op_q, &norm2, &max_norm2, &min_row}) b->free_now(); }
};
struct scan_slot { int chunk = -1, local = 0; };
struct init_share {
    pcr_ctx* ctx; const pcr_cloud_ref* clouds; const pcr_global_params* g; int host_threads;
    std::vector<chunk_plan> plans;
    size_t half = 0;                    // bytes of one half of the pinned block: chunk k is packed into half k & 1
    std::vector<scan_slot> slot;        // per row of clouds[]
    std::deque<scan_chunk> chunks;
    // PCR_INIT_TIMING: milliseconds per stage to stderr (synchronises after every stage)
    std::chrono::steady_clock::time_point t_last = std::chrono::steady_clock::now();
    void lap(const char* what) {
        static const bool timing = getenv("PCR_INIT_TIMING") != nullptr;
        if (!timing) return;
        hipStreamSynchronize(ctx->stream);
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "pcr_global_init_batch: %-28s %8.3f ms\n", what, std::chrono::duration<double, std::milli>(now - t_last).count());
        t_last = now;
    }
    float* pinned(size_t k) const { return (float*)((char*)ctx->h_init + (k & 1) * half); }
};

template <typename F>
void parallel_for(int64_t n, int threads, F&& fn) {
    if (threads > (int)n) threads = (int)n;
    if (threads <= 1) { for (int64_t i = 0; i < n; ++i) fn(i); return; }
    std::atomic<int64_t> next(0);
    auto worker = [&]() { for (;;) { const int64_t i = next.fetch_add(1); if (i >= n) break; fn(i); } };
    std::vector<std::thread> pool;
    try { for (int t = 1; t < threads; ++t) pool.emplace_back(worker); } catch (...) {}   // (a refused thread: the others do its share)
    worker();
    for (auto& th : pool) th.join();
}

// (a share of more than ~2 M points is cut into four or more chunks so that the host threads pack chunk k + 1 into the other half of
// the pinned block while the device works on chunk k)
int plan_chunks(const pcr_cloud_ref* clouds, const int64_t* scans, int64_t n_scans, std::vector<chunk_plan>* plans) {
    int64_t total = 0;
    for (int64_t s = 0; s < n_scans; ++s) {
        const pcr_cloud_ref& C = clouds[scans[s]];
        if (C.n < 0 || C.n > 0x7fffffffll || C.stride < 3 || (C.n > 0 && !C.xyz)) return PCR_E_INVALID;
        total += C.n;
    }
    int64_t chunk_pts = total / 4;
    if (chunk_pts < (2ll << 20)) chunk_pts = 2ll << 20;
    if (chunk_pts > CHUNK_PTS) chunk_pts = CHUNK_PTS;
    chunk_plan cur;
    int in_chunk = 0;
    for (int64_t s = 0; s < n_scans; ++s) {
        const int64_t n = clouds[scans[s]].n;
        if (in_chunk > 0 && (in_chunk >= CHUNK_SCANS || (int64_t)cur.at + n > chunk_pts)) {
            if (!cur.ds.empty()) plans->push_back(std::move(cur));
            cur = chunk_plan();
            in_chunk = 0;
        }
        ++in_chunk;
        if (n == 0) continue;   // (an empty scan stays without a slot: its pairs keep the identity, as when pcr_cloud_upload_f32 says PCR_E_EMPTY)
        pcr_down_scan d;
        d.first_pt = cur.at; d.n_pts = (unsigned int)n;
        cur.at += (unsigned int)n;
        cur.ds.push_back(d);
        cur.who.push_back(scans[s]);
    }
    if (!cur.ds.empty()) plans->push_back(std::move(cur));
    return PCR_OK;
}

// the context's pinned block holds two chunks of the plan (grown on demand; none of that size: PCR_E_UNSUPPORTED, the scans go one by one)
int grow_pinned(init_share& S) {
    pcr_ctx* const ctx = S.ctx;
    for (auto& P : S.plans) S.half = 12 * (size_t)P.at > S.half ? 12 * (size_t)P.at : S.half;
    S.half = (S.half + 4095) & ~(size_t)4095;
    if (S.plans.empty() || ctx->h_init_bytes >= 2 * S.half) return PCR_OK;
    if (ctx->h_init) hipHostFree(ctx->h_init);
    ctx->h_init = nullptr; ctx->h_init_bytes = 0;
    if (hipHostMalloc(&ctx->h_init, 2 * S.half, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); ctx->h_init = nullptr; return PCR_E_UNSUPPORTED; }
    ctx->h_init_bytes = 2 * S.half;
    return PCR_OK;
}

// one scan into the pinned block (3 x f32 per point, dense) + its bounding box
void pack_scan(const pcr_cloud_ref& C, float* const dst, pcr_down_scan* out) {
    const float* const src = C.xyz;
    const size_t st = (size_t)C.stride;
    float lo[12], hi[12];   // four points a trip: twelve independent minima / maxima
    for (int j = 0; j < 12; ++j) lo[j] = hi[j] = src[j % 3];
    int64_t i = 0;
    for (; i + 4 <= C.n; i += 4) {
        float v[12];
        for (int u = 0; u < 4; ++u)
            for (int d = 0; d < 3; ++d) v[3 * u + d] = src[(size_t)(i + u) * st + d];
        for (int j = 0; j < 12; ++j) {
            dst[3 * i + j] = v[j];
            lo[j] = v[j] < lo[j] ? v[j] : lo[j];
            hi[j] = v[j] > hi[j] ? v[j] : hi[j];
        }
    }
    for (; i < C.n; ++i)
        for (int d = 0; d < 3; ++d) {
            const float v = src[(size_t)i * st + d];
            dst[3 * i + d] = v;
            lo[d] = v < lo[d] ? v : lo[d];
            hi[d] = v > hi[d] ? v : hi[d];
        }
    for (int d = 0; d < 3; ++d) {
        float a = lo[d], b = hi[d];
        for (int u = 1; u < 4; ++u) { a = lo[3 * u + d] < a ? lo[3 * u + d] : a; b = hi[3 * u + d] > b ? hi[3 * u + d] : b; }
        out->mn[d] = (double)a; out->mx[d] = (double)b;
    }
}
void pack_chunk(init_share& S, size_t k) {
    chunk_plan& P = S.plans[k];
    float* const h_xyz = S.pinned(k);
    parallel_for((int64_t)P.ds.size(), S.host_threads,
                 [&](int64_t q) { pack_scan(S.clouds[P.who[(size_t)q]], h_xyz + 3 * (size_t)P.ds[(size_t)q].first_pt, &P.ds[(size_t)q]); });
}

// the matching operands of a chunk's descriptors (c.fpfh, c.scan_first, c.first, c.n_scans, c.ng are set): tile table, operands, norms.
// Reads the fail word, which synchronises: the scratch taken here -- and the caller's -- is free when this returns.
int chunk_match_operands(pcr_ctx* ctx, scan_chunk& c) {
    const size_t ng = (size_t)c.ng, ns1 = (size_t)c.n_scans + 1;
    int rc;
    c.tile_first.assign(ns1, 0u);
    for (int k = 0; k < c.n_scans; ++k) c.tile_first[(size_t)k + 1] = c.tile_first[(size_t)k] + (c.first[(size_t)k + 1] - c.first[(size_t)k] + 15u) / 16u;
    const size_t tiles = c.tile_first[(size_t)c.n_scans], op_bytes = 8 * 64 * (size_t)FM_STEPS * (tiles ? tiles : 1);
    pcr_dev_block b_tf(ctx), b_dup(ctx);
    if ((rc = b_dup.alloc(ng ? ng : 1)) || (rc = c.op_t.alloc(op_bytes)) || (rc = c.op_q.alloc(op_bytes)) || (rc = c.norm2.alloc(8 * (ng ? ng : 1))) ||
        (rc = c.max_norm2.alloc(8 * ns1)) || (rc = c.min_row.alloc(4 * ns1)) || (rc = b_tf.alloc(4 * ns1)))
        return rc;
    if (hipMemcpyAsync(b_tf.p, c.tile_first.data(), 4 * ns1, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) return PCR_E_HIP;
    if (hipMemsetAsync(c.max_norm2.p, 0, 8 * ns1, ctx->stream) != hipSuccess) return PCR_E_HIP;
    pcr_match_operands(ctx, c.fpfh.as<double>(), c.scan_first.as<unsigned int>(), c.n_scans, tiles, b_tf.as<unsigned int>(), b_dup.as<unsigned char>(), c.op_t.as<double>(),
                       c.op_q.as<double>(), c.norm2.as<double>(), c.max_norm2.as<unsigned long long>(), c.min_row.as<unsigned int>());
    if (hipGetLastError() != hipSuccess) return PCR_E_HIP;
    return pcr_read_fail(ctx);   // (synchronises: the tile table and the duplicate marks are done with)
}

// normals, SPFH, FPFH and the matching operands of a down-sampled chunk.  The per-point scratch lives to the end: read_fail synchronises.
int describe_chunk(init_share& S, scan_chunk& c) {
    pcr_ctx* const ctx = S.ctx;
    const size_t ng = (size_t)c.ng, nn = (size_t)S.g->fpfh_max_nn;
    pcr_dev_block b_nrm(ctx), b_spfh(ctx), b_id(ctx), b_d2(ctx), b_cnt(ctx);
    int rc;
    if ((rc = c.fpfh.alloc(sizeof(double) * 33 * ng)) || (rc = b_nrm.alloc(sizeof(double) * 3 * ng)) || (rc = b_spfh.alloc(sizeof(double) * 33 * ng)) ||
        (rc = b_id.alloc(sizeof(unsigned int) * nn * ng)) || (rc = b_d2.alloc(sizeof(double) * nn * ng)) || (rc = b_cnt.alloc(sizeof(int) * ng)))
        return rc;
    pcr_dev_block b_redo(ctx), b_cov(ctx);
    if ((rc = b_redo.alloc(4 * ng)) || (rc = b_cov.alloc(sizeof(double) * 7 * ng))) return rc;
    const scans_view V{c.down.as<pcr_pt>(), c.vsid.as<unsigned int>(), c.scan_first.as<unsigned int>()};
    const scans_scratch W{b_nrm.as<double>(), b_spfh.as<double>(), b_id.as<unsigned int>(), b_d2.as<double>(), b_cnt.as<int>(), b_redo.as<unsigned int>(), b_cov.as<double>()};
    if ((rc = pcr_scans_features(ctx, V, ng, S.g, W, c.fpfh.as<double>()))) return rc;
    rc = chunk_match_operands(ctx, c);   // (synchronises: the chunk's scratch and the pinned block are free for the next chunk)
    S.lap("normals + SPFH + FPFH");
    return rc;
}

// chunk k: copied to the device, down-sampled (ONE sort for all its scans), described; chunk k + 1 is packed meanwhile
int upload_chunk(init_share& S, size_t k) {
    pcr_ctx* const ctx = S.ctx;
    chunk_plan& P = S.plans[k];
    const size_t bytes = 12 * (size_t)P.at;
    std::thread packer;
    struct joiner { std::thread& t; ~joiner() { if (t.joinable()) t.join(); } } join_packer{packer};
    if (k + 1 < S.plans.size()) { try { packer = std::thread([&S, k] { pack_chunk(S, k + 1); }); } catch (...) { pack_chunk(S, k + 1); } }
    S.lap("pack (host threads)");
    pcr_dev_block b_xyz(ctx);
    int rc;
    if ((rc = b_xyz.alloc(bytes))) return rc;
    if (hipMemcpyAsync(b_xyz.p, S.pinned(k), bytes, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) return PCR_E_HIP;
    S.lap("copy to the device");
    S.chunks.emplace_back(ctx);
    scan_chunk& c = S.chunks.back();
    c.n_scans = (int)P.ds.size();
    c.first.assign(P.ds.size() + 1, 0u);
    pcr_pt* down = nullptr;
    unsigned int *vsid = nullptr, *scan_first = nullptr;
    rc = pcr_voxel_downsample_scans(ctx, (const float*)b_xyz.p, (int64_t)P.at, P.ds.data(), c.n_scans, S.g->voxel_size, &down, &vsid, &scan_first, c.first.data(), &c.ng);   // (synchronises)
    c.down.adopt(down); c.vsid.adopt(vsid); c.scan_first.adopt(scan_first);
    if (rc) return rc;
    S.lap("down-sample (all scans)");
    for (int q = 0; q < c.n_scans; ++q) {
        if (c.first[(size_t)q + 1] - c.first[(size_t)q] > (unsigned int)HYBRID_BRUTE_MAX) return PCR_E_UNSUPPORTED;
        S.slot[(size_t)P.who[(size_t)q]] = scan_slot{(int)S.chunks.size() - 1, q};
    }
    return describe_chunk(S, c);
}

// the pairs of a launch: a job per pair whose scans both hold points, and the sizes of the pool its arrays are cut from
struct job_table {
    std::vector<init_job> jobs; std::vector<int64_t> pair;   // (pair: row of pairs[] of every job)
    size_t n_i = 0, n_d = 0;     // ints / doubles of the pool
    int max_n = 1;
};
job_table build_jobs(const init_share& S, const pcr_pair_ref* pairs, const int64_t* todo, int64_t n_todo) {
    job_table tab;
    for (int64_t t = 0; t < n_todo; ++t) {
        const pcr_pair_ref& P = pairs[todo[t]];
        const scan_slot &A = S.slot[(size_t)P.src], &B = S.slot[(size_t)P.tgt];
        if (A.chunk < 0 || B.chunk < 0) continue;   // an empty scan: identity
        const scan_chunk &cs = S.chunks[(size_t)A.chunk], &ct = S.chunks[(size_t)B.chunk];
        init_job J;
        memset(&J, 0, sizeof(J));
        const unsigned int fs = cs.first[(size_t)A.local], ft = ct.first[(size_t)B.local];
        J.na = (int)(cs.first[(size_t)A.local + 1] - fs);
        J.nb = (int)(ct.first[(size_t)B.local + 1] - ft);
        if (J.na <= 0 || J.nb <= 0) continue;
        J.src = cs.down.as<pcr_pt>() + fs; J.tgt = ct.down.as<pcr_pt>() + ft;
        J.fa = cs.fpfh.as<double>() + 33 * (size_t)fs; J.fb = ct.fpfh.as<double>() + 33 * (size_t)ft;
        const size_t ts = (size_t)cs.tile_first[(size_t)A.local] * FM_STEPS * 64, tt = (size_t)ct.tile_first[(size_t)B.local] * FM_STEPS * 64;
        J.ta = cs.op_t.as<double>() + ts; J.qa = cs.op_q.as<double>() + ts; J.n2a = cs.norm2.as<double>() + fs;
        J.mxa = cs.max_norm2.as<double>() + A.local; J.mra = cs.min_row.as<unsigned int>() + A.local;
        J.tb = ct.op_t.as<double>() + tt; J.qb = ct.op_q.as<double>() + tt; J.n2b = ct.norm2.as<double>() + ft;
        J.mxb = ct.max_norm2.as<double>() + B.local; J.mrb = ct.min_row.as<unsigned int>() + B.local;
        J.seed = S.g->ransac.seed;
        // the job's part of the pool (place_jobs): ij na | ji nb | ci_ab S*na | ci_ba S*nb | corr 2 na + 4 | inl BATCH   (ints)
        //                                          dab na | dba nb | cd_ab S*na | cd_ba S*nb | err2 BATCH | Tout 12 BATCH      (doubles)
        tab.n_i += (size_t)(1 + JOB_SPLITS + 2) * J.na + (size_t)(1 + JOB_SPLITS) * J.nb + 4 + RANSAC_BATCH;
        tab.n_d += (size_t)(1 + JOB_SPLITS) * (J.na + J.nb) + 13 * (size_t)RANSAC_BATCH;
        if (J.na > tab.max_n) tab.max_n = J.na;
        if (J.nb > tab.max_n) tab.max_n = J.nb;
        tab.jobs.push_back(J);
        tab.pair.push_back(todo[t]);
    }
    return tab;
}
void place_jobs(std::vector<init_job>& jobs, int* pi, double* pd, ransac_state* ps) {
    for (auto& J : jobs) {
        J.st = ps++;
        J.ij = pi; pi += J.na;
        J.ji = pi; pi += J.nb;
        J.ci_ab = pi; pi += (size_t)JOB_SPLITS * J.na;
        J.ci_ba = pi; pi += (size_t)JOB_SPLITS * J.nb;
        J.corr = pi; J.m = pi + 2 * (size_t)J.na; pi += 2 * (size_t)J.na + 4;
        J.inl = pi; pi += RANSAC_BATCH;
        J.dab = pd; pd += J.na;
        J.dba = pd; pd += J.nb;
        J.cd_ab = pd; pd += (size_t)JOB_SPLITS * J.na;
        J.cd_ba = pd; pd += (size_t)JOB_SPLITS * J.nb;
        J.err2 = pd; pd += RANSAC_BATCH;
        J.Tout = pd; pd += 12 * (size_t)RANSAC_BATCH;
    }
}

// the RANSAC loop of every job: the first batch for all of them, then batch by batch for those still running (d_act: scratch for their
// indices); the transform of every job with a valid hypothesis goes to its pair's row of T_init
int ransac_jobs(init_share& S, const job_table& tab, const init_job* d_jobs, const ransac_state* d_st, int* d_act, double* T_init) {
    pcr_ctx* const ctx = S.ctx;
    const int nj = (int)tab.jobs.size(), max_iteration = S.g->ransac.max_iteration;
    ransac_common c = ransac_common_of(&S.g->ransac);
    std::vector<ransac_state> st((size_t)nj);
    std::vector<int> active;
    int rc;
    for (long long done = 0; done < max_iteration; done += c.n_iter) {
        c.first_iter = (int)done; c.n_iter = ransac_batch_size(done, max_iteration);
        const int n_run = done == 0 ? nj : (int)active.size();
        if (done > 0 && hipMemcpyAsync(d_act, active.data(), 4 * (size_t)n_run, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) return PCR_E_HIP;
        pcr_ransac_jobs_round(ctx, d_jobs, done == 0 ? nullptr : d_act, n_run, c);
        if (hipGetLastError() != hipSuccess) return PCR_E_HIP;
        if ((rc = pcr_d2h_staged(ctx, st.data(), d_st, sizeof(ransac_state) * (size_t)nj))) return rc;   // every job's state, one read (synchronises)
        active.clear();
        for (int j = 0; j < nj; ++j)
            if (!st[(size_t)j].stop) active.push_back(j);
        S.lap("RANSAC round");
        if (active.empty()) break;
    }
    for (int j = 0; j < nj; ++j) {
        const ransac_state& h = st[(size_t)j];
        if (h.m < 3 || h.best_itr < 0) continue;   // PCR_E_TOO_FEW_ASSOC pair by pair: identity
        double* T = T_init + 16 * (size_t)tab.pair[(size_t)j];
        for (int k = 0; k < 16; ++k) T[k] = (k % 5 == 0) ? 1.0 : 0.0;
        ransac_T16(h.bestT, T);
    }
    return PCR_OK;
}

// the device side of a job table: the pool its arrays are cut from, the jobs, the list of running ones, their loop states
struct job_pool {
    pcr_dev_block b_i, b_d, b_jobs, b_act, b_st;
    explicit job_pool(pcr_ctx* c) : b_i(c), b_d(c), b_jobs(c), b_act(c), b_st(c) {}
};
// matching both ways, correspondence set and initial loop state of every job of the table (enqueued; tab.jobs gets the device addresses)
int match_jobs(pcr_ctx* ctx, job_table& tab, job_pool& P, int mutual, int max_iteration) {
    const int nj = (int)tab.jobs.size();
    int rc;
    if ((rc = P.b_i.alloc(4 * tab.n_i)) || (rc = P.b_d.alloc(8 * tab.n_d)) || (rc = P.b_jobs.alloc(sizeof(init_job) * nj)) || (rc = P.b_act.alloc(4 * (size_t)nj)) ||
        (rc = P.b_st.alloc(sizeof(ransac_state) * (size_t)nj)))
        return rc;
    place_jobs(tab.jobs, P.b_i.as<int>(), P.b_d.as<double>(), P.b_st.as<ransac_state>());
    if (hipMemcpyAsync(P.b_jobs.p, tab.jobs.data(), sizeof(init_job) * nj, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) return PCR_E_HIP;
    pcr_match_jobs(ctx, P.b_jobs.as<init_job>(), nj, tab.max_n, mutual, max_iteration);
    return PCR_OK;
}

// matching, correspondence sets and RANSAC of up to PAIR_CHUNK pairs side by side
int register_pairs(init_share& S, const pcr_pair_ref* pairs, const int64_t* todo, int64_t n_todo, double* T_init) {
    pcr_ctx* const ctx = S.ctx;
    job_table tab = build_jobs(S, pairs, todo, n_todo);
    if (tab.jobs.empty()) return PCR_OK;
    job_pool P(ctx);
    int rc;
    if ((rc = match_jobs(ctx, tab, P, S.g->mutual_filter ? 1 : 0, S.g->ransac.max_iteration))) return rc;
    S.lap("matching + correspondences");
    return ransac_jobs(S, tab, P.b_jobs.as<init_job>(), P.b_st.as<ransac_state>(), P.b_act.as<int>(), T_init);
}
}  // namespace

int pcr_global_init_batch(pcr_ctx* ctx, const pcr_cloud_ref* clouds, int64_t n_clouds, const int64_t* scans, int64_t n_scans, const pcr_pair_ref* pairs,
                          const int64_t* todo, int64_t n_todo, const pcr_global_params* g, double* T_init, int host_threads) {
    if (!ctx || !clouds || !scans || !pairs || !todo || !g || !T_init || n_scans < 1 || n_todo < 1) return PCR_E_INVALID;
    if (!prep_params_ok(g->voxel_size, g->normal_radius, g->normal_max_nn, g->fpfh_radius, g->fpfh_max_nn) || !ransac_params_ok(&g->ransac)) return PCR_E_INVALID;
    if (getenv("PCR_INIT_PER_SCAN") != nullptr) return PCR_E_UNSUPPORTED;   // A/B and tests: the scans one by one (read per call)
    hipSetDevice(ctx->device);
    init_share S{ctx, clouds, g, host_threads};
    S.slot.resize((size_t)n_clouds);
    int rc = plan_chunks(clouds, scans, n_scans, &S.plans);
    if (rc == PCR_OK) rc = grow_pinned(S);
    if (rc) return rc;
    if (!S.plans.empty()) pack_chunk(S, 0);
    for (size_t k = 0; k < S.plans.size() && rc == PCR_OK; ++k) rc = upload_chunk(S, k);
    for (int64_t p0 = 0; p0 < n_todo && rc == PCR_OK; p0 += PAIR_CHUNK)
        rc = register_pairs(S, pairs, todo + p0, p0 + PAIR_CHUNK < n_todo ? PAIR_CHUNK : n_todo - p0, T_init);
    pcr_sync(ctx->stream);
    while (!S.chunks.empty()) S.chunks.pop_front();   // (first to last, behind the synchronisation)
    return rc;
}

// Diagnostic entry point (include/pcr.h): the fused path's matching alone, on descriptor sets the caller brings.  The sets become one
// chunk whose "scans" they are -- operands by chunk_match_operands, jobs by build_jobs / match_jobs, as upload_chunk and register_pairs do.
extern "C" int pcr_match_pairs_fused(pcr_ctx* ctx, const double* descriptors, const int64_t* set_first, int64_t n_sets, const int32_t* pair_sets, int64_t n_pairs,
                                     int mutual_filter, int32_t* ij_out, double* dab_out, int32_t* ji_out, double* dba_out, int32_t* corr_out, int32_t* m_out) {
    if (!ctx || !descriptors || !set_first || !pair_sets || !ij_out || !dab_out || !ji_out || !dba_out || !corr_out || !m_out) return PCR_E_INVALID;
    if (n_sets < 1 || n_sets > CHUNK_SCANS || n_pairs < 1 || set_first[0] != 0) return PCR_E_INVALID;
    for (int64_t s = 0; s < n_sets; ++s) {
        if (set_first[s + 1] <= set_first[s]) return PCR_E_INVALID;
        if (set_first[s + 1] - set_first[s] > HYBRID_BRUTE_MAX) return PCR_E_UNSUPPORTED;
    }
    for (int64_t p = 0; p < 2 * n_pairs; ++p)
        if (pair_sets[p] < 0 || pair_sets[p] >= n_sets) return PCR_E_INVALID;
    hipSetDevice(ctx->device);
    pcr_global_params g;
    pcr_global_default_params(2.0, &g);
    init_share S{ctx, nullptr, &g, 1};
    S.slot.resize((size_t)n_sets);
    S.chunks.emplace_back(ctx);
    scan_chunk& c = S.chunks.back();
    c.ng = set_first[n_sets]; c.n_scans = (int)n_sets;
    c.first.resize((size_t)n_sets + 1);
    for (int64_t s = 0; s <= n_sets; ++s) c.first[(size_t)s] = (unsigned int)set_first[s];
    for (int64_t s = 0; s < n_sets; ++s) S.slot[(size_t)s] = scan_slot{0, (int)s};
    const size_t ng = (size_t)c.ng;
    int rc;
    // (no points behind these descriptors: the records a job's RANSAC would sample stay zero, and no RANSAC runs)
    if ((rc = c.down.alloc(sizeof(pcr_pt) * ng)) || (rc = c.scan_first.alloc(4 * ((size_t)n_sets + 1))) || (rc = c.fpfh.alloc(sizeof(double) * 33 * ng))) return rc;
    PCR_HIP(ctx, hipMemsetAsync(c.down.p, 0, sizeof(pcr_pt) * ng, ctx->stream));
    PCR_HIP(ctx, hipMemcpyAsync(c.scan_first.p, c.first.data(), 4 * ((size_t)n_sets + 1), hipMemcpyHostToDevice, ctx->stream));
    PCR_HIP(ctx, hipMemcpyAsync(c.fpfh.p, descriptors, sizeof(double) * 33 * ng, hipMemcpyHostToDevice, ctx->stream));
    if ((rc = chunk_match_operands(ctx, c))) return rc;
    std::vector<pcr_pair_ref> pairs((size_t)n_pairs);
    std::vector<int64_t> todo((size_t)n_pairs);
    for (int64_t p = 0; p < n_pairs; ++p) { pairs[(size_t)p].src = pair_sets[2 * p]; pairs[(size_t)p].tgt = pair_sets[2 * p + 1]; pairs[(size_t)p].T0 = nullptr; todo[(size_t)p] = p; }
    std::vector<size_t> at_a((size_t)n_pairs + 1, 0), at_b((size_t)n_pairs + 1, 0);   // where a pair's rows start in the outputs
    for (int64_t p = 0; p < n_pairs; ++p) {
        at_a[(size_t)p + 1] = at_a[(size_t)p] + (size_t)(set_first[pair_sets[2 * p] + 1] - set_first[pair_sets[2 * p]]);
        at_b[(size_t)p + 1] = at_b[(size_t)p] + (size_t)(set_first[pair_sets[2 * p + 1] + 1] - set_first[pair_sets[2 * p + 1]]);
    }
    for (int64_t p0 = 0; p0 < n_pairs; p0 += PAIR_CHUNK) {
        job_table tab = build_jobs(S, pairs.data(), todo.data() + p0, p0 + PAIR_CHUNK < n_pairs ? PAIR_CHUNK : n_pairs - p0);
        job_pool P(ctx);
        if ((rc = match_jobs(ctx, tab, P, mutual_filter ? 1 : 0, 1))) return rc;
        PCR_HIP(ctx, hipGetLastError());
        for (size_t j = 0; j < tab.jobs.size(); ++j) {   // (every set holds rows: a job per pair, in order)
            const init_job& J = tab.jobs[j];
            const size_t p = (size_t)tab.pair[j], a = at_a[p], b = at_b[p];
            PCR_HIP(ctx, hipMemcpyAsync(ij_out + a, J.ij, 4 * (size_t)J.na, hipMemcpyDeviceToHost, ctx->stream));
            PCR_HIP(ctx, hipMemcpyAsync(dab_out + a, J.dab, 8 * (size_t)J.na, hipMemcpyDeviceToHost, ctx->stream));
            if (mutual_filter) {
                PCR_HIP(ctx, hipMemcpyAsync(ji_out + b, J.ji, 4 * (size_t)J.nb, hipMemcpyDeviceToHost, ctx->stream));
                PCR_HIP(ctx, hipMemcpyAsync(dba_out + b, J.dba, 8 * (size_t)J.nb, hipMemcpyDeviceToHost, ctx->stream));
            }
            PCR_HIP(ctx, hipMemcpyAsync(corr_out + 2 * a, J.corr, 8 * (size_t)J.na, hipMemcpyDeviceToHost, ctx->stream));
            PCR_HIP(ctx, hipMemcpyAsync(m_out + p, J.m, 4, hipMemcpyDeviceToHost, ctx->stream));
        }
        PCR_HIP(ctx, pcr_sync(ctx->stream));   // (before the pool goes back)
    }
    while (!S.chunks.empty()) S.chunks.pop_front();
    return PCR_OK;
}
