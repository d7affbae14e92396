// hz_api_horizon.hip -- the horizon drivers behind the C ABI (include/horayzon_hip.h): hz_horizon_gridded* and its
// per-scene, planes, 16-bit and "with distances" forms (horizon_run), hz_horizon_locations* (locations_run),
// hz_horizon_distance* (horidist_run), hz_horizon_tables.
//
// Host-side driver logic restating horizon_gridded_comp (horizon_comp.cpp:629-822): unit conversions, trig tables with the
// reference's float/double promotion pattern, uploads, kernel launches, reports.
#include "hz_internal.h"
#include <cmath>
#include <cstring>
#include <vector>
#include <thread>
#include <atomic>
#include <utility>

namespace hz {

struct HostTables {
    std::vector<float> azim_sin, azim_cos, elev_ang, elev_sin, elev_cos;
    std::vector<int> mid_idx;   // (index nearest to the midpoint of entries i and i + 10, bits of elev_ang[that index]) (horizon_comp.cpp:462-464)
    int elev_num = 0;
    float hori_acc = 0, low = 0, up = 0;
};

// horizon_comp.cpp:648, :667-669, :711-731
static void build_tables(int azim_num, float hori_acc_deg, float low_deg, HostTables &t) {
    float elev_ang_up_lim = 89.98;
    t.hori_acc = deg2rad_f(hori_acc_deg);
    t.low = deg2rad_f(low_deg);
    t.up = deg2rad_f(elev_ang_up_lim);
    t.azim_sin.resize((size_t)azim_num); t.azim_cos.resize((size_t)azim_num);
    float ang;
    for (int i = 0; i < azim_num; i++) {
        ang = (float)(((2 * M_PI) / azim_num) * i);
        t.azim_sin[(size_t)i] = sinf(ang);
        t.azim_cos[(size_t)i] = cosf(ang);
    }
    const double step = (double)t.hori_acc / 5.0;
    t.elev_num = (int)ceil((double)(t.up - t.low) / step) + 1;
    const size_t n = (size_t)std::max(t.elev_num, 0);
    t.elev_ang.resize(n); t.elev_sin.resize(n); t.elev_cos.resize(n);
    for (int i = 0; i < t.elev_num; i++) {
        ang = (float)((double)t.up - step * (double)i);
        t.elev_ang[(size_t)(t.elev_num - i - 1)] = ang;
        t.elev_sin[(size_t)(t.elev_num - i - 1)] = sinf(ang);
        t.elev_cos[(size_t)(t.elev_num - i - 1)] = cosf(ang);
    }
    // elev_samp = (elev_ang[prev] + elev_ang[ind]) / 2.0; ind = (int)roundf((elev_samp - low) / (hori_acc / 5.0))
    // (stored as pairs: the index and the bits of elev_ang[index], the value the search emits -- one 8 B load instead of
    //  two dependent 4 B loads at the end of every azimuth)
    t.mid_idx.assign(2 * (n > 0 ? n : 1), 0);
    for (int i = 0; i + 10 < t.elev_num; i++) {
        const float es = (float)((double)(t.elev_ang[(size_t)i] + t.elev_ang[(size_t)i + 10]) / 2.0);
        const int mid = (int)roundf((float)((double)(es - t.low) / step));
        t.mid_idx[2 * (size_t)i] = mid;
        const float ev = t.elev_ang[(size_t)std::min(std::max(mid, 0), t.elev_num - 1)];
        memcpy(&t.mid_idx[2 * (size_t)i + 1], &ev, sizeof(float));
    }
}

static int parse_alg(const char *s, int *alg) {
    if (s && strcmp(s, "discrete_sampling") == 0) { *alg = 0; return HZ_OK; }
    if (s && strcmp(s, "binary_search") == 0) { *alg = 1; return HZ_OK; }
    if (s && strcmp(s, "guess_constant") == 0) { *alg = 2; return HZ_OK; }
    return set_error(HZ_ERR_ARG, "invalid input argument for ray_algorithm");
}

// Host output of the drop-in call (NumPy memory, pageable): a device-to-host copy into pageable memory is staged by the
// runtime (copy kernels on the CUs, host-blocking, 16 GB/s into untouched pages -- scripts/d2h_probe.py) and slows the
// traversal kernel it is meant to hide behind.  HostPinner page-locks the caller's slab region by region (one region per
// chunk of rows) on a helper thread, ahead of the copies: 45 ms per GB, done while the first chunks are traced; the copies
// are then plain DMA (57 GB/s, no CU time).
// Only pages that lie WHOLLY inside the slab are ever registered (the first region starts at the first page boundary at or
// after the slab's first byte, the last one ends at the last boundary at or before its end): a neighbouring slab of the
// same array -- horizon.py's devices=[...] path runs one call per GPU on adjacent slabs of one NumPy array -- never sees one
// of its pages registered or unregistered by somebody else.  The unaligned head and tail (< 4096 B each) go as pageable
// copies of their own.  Regions are page aligned and disjoint; a copy is cut at every region boundary it contains (a copy
// must not straddle two separately registered ranges, nor a registered and a pageable one) and waits for every region it
// touches.  If page locking fails (memlock limit, memory that is already registered) the remaining regions stay pageable.
// Outputs below 8 MiB are not pinned at all: the thread and the registration cost more than they save.
struct HostPinner {
    std::vector<std::pair<char *, size_t>> regions;      // what is (still) registered: the worker zeroes a size on failure
    std::vector<std::pair<char *, size_t>> planned;      // the same list as laid out by start()
    std::atomic<int> done{0};
    std::atomic<bool> failed{false};
    std::thread worker;
    int device = 0;
    void start(int dev, char *base, const std::vector<size_t> &chunk_bytes) {
        device = dev;
        const uintptr_t page = 4096;
        size_t total = 0;
        for (size_t b : chunk_bytes) total += b;
        if (total < ((size_t)8 << 20)) return;
        const uintptr_t first = reinterpret_cast<uintptr_t>(base);
        const uintptr_t last_page = (first + total) & ~(page - 1);          // end of the last whole page inside the slab
        uintptr_t lo = (first + page - 1) & ~(page - 1);                    // first whole page inside the slab
        uintptr_t cur = first;
        for (size_t k = 0; k < chunk_bytes.size(); k++) {
            cur += chunk_bytes[k];
            const uintptr_t hi = std::min(cur & ~(page - 1), last_page);
            regions.emplace_back(reinterpret_cast<char *>(lo), hi > lo ? (size_t)(hi - lo) : 0);
            lo = std::max(lo, hi);
        }
        planned = regions;
        worker = std::thread([this]() {
            (void)hipSetDevice(device);
            for (size_t k = 0; k < regions.size(); k++) {
                if (!failed.load() && regions[k].second &&
                    hipHostRegister(regions[k].first, regions[k].second, hipHostRegisterDefault) != hipSuccess) {
                    (void)hipGetLastError();
                    regions[k].second = 0;               // not ours to unregister
                    failed.store(true);
                } else if (failed.load()) {
                    regions[k].second = 0;
                }
                done.store((int)k + 1, std::memory_order_release);
            }
        });
    }
    // Wait until every region that overlaps [dst, dst + bytes) is locked (or locking has been given up), then return the
    // offsets at which a copy of that range has to be cut: every region boundary strictly inside it.
    std::vector<size_t> cuts_for(const char *dst, size_t bytes) const {
        std::vector<size_t> cuts;
        int need = 0;
        for (size_t k = 0; k < planned.size(); k++) {          // `planned` is immutable once the worker runs
            const char *lo = planned[k].first, *hi = lo + planned[k].second;
            if (planned[k].second && hi > dst && lo < dst + bytes) need = (int)k + 1;
        }
        while (done.load(std::memory_order_acquire) < need) std::this_thread::yield();
        for (int k = 0; k < need; k++) {                       // regions[k] is final for k < done (release / acquire)
            const char *lo = planned[(size_t)k].first, *hi = lo + planned[(size_t)k].second;
            if (planned[(size_t)k].second == 0) continue;
            if (lo > dst && lo < dst + bytes) cuts.push_back((size_t)(lo - dst));
            if (hi > dst && hi < dst + bytes) cuts.push_back((size_t)(hi - dst));
        }
        std::sort(cuts.begin(), cuts.end());
        cuts.erase(std::unique(cuts.begin(), cuts.end()), cuts.end());
        return cuts;
    }
    void finish() {          // after every copy has completed
        if (worker.joinable()) worker.join();
        for (auto &r : regions) if (r.second) (void)hipHostUnregister(r.first);
        regions.clear();
    }
    ~HostPinner() { finish(); }
};

// The certificate monitor of opts.verify_near without count_work: see horizon_run.
struct NearMonitor {
    int device = 0;
    hipStream_t st_mon = nullptr;
    hipEvent_t ready = nullptr, done = nullptr;
    void *buf = nullptr;
    size_t buf_bytes = 0;
    unsigned long long *cnt = nullptr;
    bool active = false;
    int launch(const Scene *sc, const HorizonArgs &a, int n, int seed, hipStream_t st) {
        device = sc->device;
        const int nb = horizon_num_blocks(a);
        std::vector<int> pick;
        for (int b = 0; b < nb; b++) {
            uint32_t h = (uint32_t)b * 2654435761u + (uint32_t)seed * 40503u;
            h ^= h >> 15; h *= 2246822519u; h ^= h >> 13;
            if (h % (uint32_t)n == 0u) pick.push_back(b);
        }
        if (pick.empty()) return HZ_OK;
        int rc;
        if (!st_mon && (rc = stream_acquire(device, &st_mon))) return rc;
        if (!ready) { HZ_HIP(hipEventCreateWithFlags(&ready, hipEventDisableTiming)); HZ_HIP(hipEventCreateWithFlags(&done, hipEventDisableTiming)); }
        const size_t cbytes = HZ_CNT_N * sizeof(unsigned long long) + HZ_REDO_CAP * sizeof(int);
        const size_t row_bytes = ((size_t)a.azim_num * sizeof(float) + 255) & ~(size_t)255;     // the scratch row its stores go to
        const size_t need = cbytes + row_bytes + pick.size() * sizeof(int);
        if (need > buf_bytes) {                               // (allocated once per call: the chunks of a call pick about as many blocks)
            if (buf) { (void)hipFree(buf); buf = nullptr; buf_bytes = 0; }
            HZ_HIP(hipMalloc(&buf, need + need / 4));
            buf_bytes = need + need / 4;
        }
        cnt = (unsigned long long *)buf;
        float *scratch = (float *)((char *)buf + cbytes);
        int *d_list = (int *)((char *)buf + cbytes + row_bytes);
        HZ_HIP(hipEventRecord(ready, st));                    // certificates (and everything enqueued before) are complete
        HZ_HIP(hipStreamWaitEvent(st_mon, ready, 0));
        HZ_HIP(hipMemsetAsync(buf, 0, cbytes, st_mon));
        HZ_HIP(hipMemcpyAsync(d_list, pick.data(), pick.size() * sizeof(int), hipMemcpyHostToDevice, st_mon));
        HZ_HIP(hipStreamSynchronize(st_mon));                 // `pick` is host memory of this scope; the copy is tiny
        HorizonArgs v = a;
        v.count_work = 1; v.verify_near = 1; v.level_stack = 1;
        v.scratch_row = scratch;                              // its stores must not land in the production launch's rows
        v.counters = cnt; v.tile_list = d_list; v.n_list = (int)pick.size();
        if ((rc = horizon_launch(sc, v, st_mon, nullptr))) return rc;
        HZ_HIP(hipEventRecord(done, st_mon));
        active = true;
        return HZ_OK;
    }
    // the production stream waits for the monitor (later kernels read the rows it rewrote); tallies are added up
    int collect(hipStream_t st, unsigned long long *verified, unsigned long long *violations) {
        unsigned long long c2[HZ_CNT_N] = {0};
        HZ_HIP(hipStreamWaitEvent(st, done, 0));
        HZ_HIP(hipMemcpyAsync(c2, cnt, sizeof(c2), hipMemcpyDeviceToHost, st_mon));
        HZ_HIP(hipStreamSynchronize(st_mon));
        *verified += c2[HZ_CNT_VERIFIED]; *violations += c2[HZ_CNT_VIOLATIONS];
        active = false;
        return HZ_OK;
    }
    ~NearMonitor() {
        if (st_mon) { (void)hipSetDevice(device); stream_release(device, st_mon); }
        if (ready) (void)hipEventDestroy(ready);
        if (done) (void)hipEventDestroy(done);
        if (buf) (void)hipFree(buf);
    }
};

// opts.verbose >= 2: why cells got no certificate (device histogram of hz_near.hip), to stderr
static void print_near_reasons(const unsigned *near_reasons) {
    unsigned h[20] = {0};
    if (hipMemcpy(h, near_reasons, sizeof(h), hipMemcpyDeviceToHost) != hipSuccess) { (void)hipGetLastError(); return; }
    static const char *nm[14] = {"frame", "vertex_on_axis", "edge_over_axis", "az_tolerance", "inplane_edge", "crossing_near_axis",
                                 "interval", "precision", "edge_on", "orientation", "origin_below", "axis_in_triangle", "window_or_mask",
                                 "bad_mesh_nearby"};
    fprintf(stderr, "hz near reasons: cells %u certified %u", h[0], h[1]);
    for (int b = 0; b < 14; b++) if (h[2 + b]) fprintf(stderr, " %s %u", nm[b], h[2 + b]);
    fprintf(stderr, " | tasks %u bins %u\n", h[16], h[17]);
}

// opts.verbose: the reference's report, horizon_comp.cpp:673-700, 805-810 (same lines, same order)
static void print_reference_report(const Scene *sc, int alg, unsigned long long cells, unsigned long long rays, size_t slab_cells,
                                   int dim_in_0, int dim_in_1, int azim_num, double kernel_s, bool certificates_off, bool certificates_per_cell) {
    static const char *alg_name[3] = {"discrete_sampling", "binary search", "guess horizon from previous azimuth direction"};
    printf("Horizon detection algorithm: %s\n", alg_name[alg]);
    printf("Number of grid cells for which horizon is computed: %llu \n", cells);
    printf("Fraction of total number of grid cells: %g %%\n", (double)((float)cells / (float)slab_cells * 100.0f));
    printf("Total memory required for horizon output: %g GB\n",
           (double)(((float)dim_in_0 * (float)dim_in_1 * (float)azim_num * 4.0f) / 1.0e9f));
    printf("Ray tracing time: %g s\n", kernel_s);
    printf("Number of rays shot: %llu\n", rays);
    printf("Average number of rays per location and azimuth: %.2f \n",
           cells ? (double)((float)rays / (float)(cells * (unsigned long long)azim_num)) : 0.0);
    // (not a line of the reference: why this call ran without the near-field certificates, if it did)
    if (certificates_off)
        printf("Near-field certificates off: a DEM quad that is not part of a height field over the (x, y) plane, or a triangle "
               "of the outer simplified domain, is too large for the per-cell guard (results unaffected, slower)\n");
    else if (certificates_per_cell)
        printf("Near-field certificates per cell: %u DEM triangle(s) project onto the (x, y) plane collapsed or against the "
               "majority, %d outer-domain triangle(s); cells near them run without (results unaffected)\n", sc->hdr.n_flipped, sc->hdr.n_tin);
    fflush(stdout);
}

// the tables of build_tables on the device (mid_idx only where a search reads it)
struct DevTables {
    DevIn<float> azim_sin, azim_cos, elev_ang, elev_sin, elev_cos;
    DevIn<int> mid_idx;
    int bind(const HostTables &t, bool with_mid, hipStream_t st) {
        int rc;
        const size_t A = t.azim_sin.size(), E = (size_t)t.elev_num;
        if ((rc = azim_sin.bind(t.azim_sin.data(), A, st)) || (rc = azim_cos.bind(t.azim_cos.data(), A, st)) ||
            (rc = elev_ang.bind(t.elev_ang.data(), E, st)) || (rc = elev_sin.bind(t.elev_sin.data(), E, st)) ||
            (rc = elev_cos.bind(t.elev_cos.data(), E, st))) return rc;
        return with_mid ? mid_idx.bind(t.mid_idx.data(), t.mid_idx.size(), st) : HZ_OK;
    }
};

// Rows per launch and the device buffer of one chunk of horizon, when `hori` is host memory or skipped (SVF only).
// Every launch ends with a tail (the last waves run on a draining GPU; a lane owns its cell for all azimuths), so launches
// should be few: at least 16 GiB of horizon per launch when it is only the SVF's input (nothing is copied out; less if HBM is
// short), at least 4 GiB when chunks are copied to the host behind the next chunk's kernel.  The row arithmetic is
// horizon_chunk_rows (hz_horizon_plan.h); here the byte target is chosen and halved until hipMalloc succeeds.
static int alloc_hori_chunk(int rows_all, size_t row_bytes, bool skip_hori, int fixed_rows, int *chunk_rows_out, DevBuf *buf) {
    size_t target = skip_hori ? ((size_t)16 << 30) : ((size_t)4 << 30);
    {   // host path with plenty of free HBM: equal chunks of <= 8 GiB (the 3601^2 tile: 3 instead of 5 launches, 2.57 ->
        // 2.49 s).  (64 GiB chunks for the SVF-only path were measured on config 5: 5 instead of 18 launches save
        // 0.7 s of kernel tails and cost 2 s of hipMalloc / hipFree of the 62 + 33 GB buffers -- kept at 16 GiB.)
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
            if (!skip_hori) {
                const size_t all = (size_t)rows_all * row_bytes;
                const size_t parts = std::max<size_t>(1, (all + ((size_t)8 << 30) - 1) / ((size_t)8 << 30));
                if (free_b / 6 >= all / parts + row_bytes) target = std::max(target, all / parts + row_bytes);
            }
        } else (void)hipGetLastError();
    }
    for (;;) {
        const int chunk_rows = horizon_chunk_rows(rows_all, row_bytes, target, fixed_rows);
        *chunk_rows_out = chunk_rows;
        if (buf->alloc((size_t)chunk_rows * row_bytes) == hipSuccess) return HZ_OK;
        (void)hipGetLastError();
        buf->p = nullptr;
        if (fixed_rows > 0 || target <= ((size_t)1 << 30)) return set_error(HZ_ERR_HIP, "hipMalloc of the horizon chunk (%zu bytes) failed", (size_t)chunk_rows * row_bytes);
        target >>= 1;
    }
}

// the certificate scratch kept with the scene, grown to hold `cells` cells ((2 A + 4) B per cell)
static int grow_near_scratch(const Scene *sc, size_t cells, int azim_num) {
    if (!Scene::grow_scratch(sc->near_buf, sc->near_bytes, near_scratch_bytes(cells, azim_num)))
        return set_error(HZ_ERR_HIP, "hipMalloc of the near-field certificates failed");
    return HZ_OK;
}

// Near-field certificates of the rows [na.row_begin, na.row_end) (hz_near.hip) into the scratch kept with the scene; fills
// na.near_idx / near_r, adds the pre-pass's GPU time to *ms_near.
static int near_prepass(const Scene *sc, NearArgs &na, hipStream_t st, float *ms_near) {
    const size_t cells = (size_t)(na.row_end - na.row_begin) * na.dim_in_1;
    int rc = grow_near_scratch(sc, cells, na.azim_num);
    if (rc) return rc;
    na.near_idx = (unsigned short *)sc->near_buf;
    na.near_r = (float *)((char *)sc->near_buf + near_idx_bytes(cells, na.azim_num));
    Event begin, end;
    if ((rc = begin.record(st))) return rc;
    rc = near_launch(sc, na, st);
    const int rc_end = end.record(st);
    if (!rc && !rc_end) {
        (void)hipEventSynchronize(end.e);
        *ms_near += begin.ms_until(end);
    }
    return rc ? rc : rc_end;
}

// Leftover cells (hz_horizon.hip): a block of a production launch ends when at most t[0] (default 36; opts.left_min) of its cells are
// unfinished -- a lane whose cell is done idles until its block's slowest cell is (12 % of the lane time, profiles/r05/
// probe_done_lanes.log) -- and follow-up launches finish the cells handed over, 64 per wave, sorted by the azimuths they have left
// and by position (left_sort); a wave of follow-up launch l may hand over again at t[l], the last one runs to the end.  How many
// records a level got is only known on the device: keys, sort and follow-up launches are sized by the region's capacity and read
// the counts there, the host never waits between them.  The regions are laid out by left_plan (hz_horizon_plan.h); a region that
// still runs out of room stops the hand-over (hz_horizon.hip).  Kept with the scene.
// Fills left_t[] (thresholds per level) and a.left_base / left_cap / left_sort / left_cap_max, grows the scene's buffer; returns the
// number of follow-up launches (0: no hand-over -- switched off, a counting call, or no memory: the blocks run to their end).
static int plan_leftover(const Scene *sc, const hz_opts *opts, int rows_max, int dim_in_1, int left_t[HZ_LEFT_LEVELS], HorizonArgs &a) {
    const int n_left_launches = left_thresholds(opts ? opts->left_min : 0, left_t);
    if ((opts && opts->count_work) || n_left_launches == 0) return 0;
    const TileMap tm = make_tile_map((rows_max + 15) / 16, (dim_in_1 + 15) / 16);
    const LeftPlan lp = left_plan(left_t, n_left_launches, tm.per_xcd, opts ? opts->left_cap_test : 0, sort_temp_elems);
    for (int l = 0; l < n_left_launches; l++) { a.left_base[l] = lp.left_base[l]; a.left_cap[l] = lp.left_cap[l]; }
    // (record numbers and launch-local cell numbers are 32 bit)
    if (!lp.on || (unsigned long long)rows_max * (unsigned long long)dim_in_1 >= 0xffffffffull) return 0;
    if (!Scene::grow_scratch(sc->left_buf, sc->left_bytes, lp.total_bytes)) return 0;
    a.left_sort = (uint32_t *)((char *)sc->left_buf + lp.rec_bytes); a.left_cap_max = lp.cap_max;
    return n_left_launches;
}

// ---- one gridded horizon call ---------------------------------------------------------------------------------------------
// The output: `hori` in the layout hori_kind names (HZ_HORI_PLANES / HZ_HORI_U16, include/horayzon_hip.h; 0: the reference's
// float32 [rows][dim_in_1][azim_num]), device or host memory; `dist` (null: not wanted) float32 in the layout the planes bit
// names.  hori == nullptr together with opts->skip_hori is the call that returns the maps only.
struct HoriOut {
    void *hori = nullptr;
    int hori_kind = 0;
    float *dist = nullptr;
};

struct HorizonCall {
    const float *vec_norm, *vec_north;
    int offset_0, offset_1, dim_in_0, dim_in_1, azim_num;
    float dist_search, hori_acc;
    const char *ray_algorithm;
    float elev_ang_low_lim;
    const uint8_t *mask;
    float hori_fill, ray_org_elev;
    const hz_opts *opts;
    const hz_topo_out *topo;
    hz_stats *stats;
    HoriOut out;
};

// what check_horizon_call resolves
struct HorizonWants {
    int alg = 2;
    int row_begin = 0, row_end = 0;      // the row slab; begin == end: nothing to do
    bool skip_hori = false;
    bool to_planes = false;              // the horizon leaves as planes[azim][y][x]: the cell-major horizon lives in the chunk buffer of skip_hori
                                         // only, and every chunk is transposed into its rows of every plane (hz_planes.hip)
    bool to_q16 = false;                 // the horizon leaves as 16-bit codes (hz_q16.hip), cell-major or as planes: the float32 horizon lives in
                                         // the same chunk buffer, is reduced there (svf, topo) and then encoded into its place
    bool want_dist = false;              // the distance to the horizon (hz_horidist.hip) of every chunk, from the float32 chunk on the device
    bool want_svf = false, want_vsf = false, want_open = false;
};

// row slab (include/horayzon_hip.h): {0, 0} = the whole inner domain (a zeroed struct), row_end == -1 = dim_in_0, anything else
// must satisfy 0 <= row_begin <= row_end <= dim_in_0; begin == end is an empty slab: nothing to do
static int resolve_row_slab(const hz_opts *opts, int dim_in_0, int *row_begin, int *row_end) {
    *row_begin = 0; *row_end = dim_in_0;
    if (!opts || (opts->row_begin == 0 && opts->row_end == 0)) return HZ_OK;
    *row_begin = opts->row_begin;
    *row_end = (opts->row_end == -1) ? dim_in_0 : opts->row_end;
    if (*row_begin < 0 || *row_end < 0 || *row_end > dim_in_0 || *row_begin > *row_end)
        return set_error(HZ_ERR_ARG, "invalid row slab [%d, %d) for dim_in_0 = %d", opts->row_begin, opts->row_end, dim_in_0);
    return HZ_OK;
}

static int check_horizon_call(const Scene *sc, const HorizonCall &c, HorizonWants *w) {
    const hz_opts *opts = c.opts;
    const hz_topo_out *topo = c.topo;
    const int rc = parse_alg(c.ray_algorithm, &w->alg);
    if (rc) return rc;
    if (!c.vec_norm || !c.vec_north || !c.mask) return set_error(HZ_ERR_ARG, "vec_norm, vec_north and mask must not be NULL");
    if (c.dim_in_0 <= 0 || c.dim_in_1 <= 0 || c.azim_num <= 0) return set_error(HZ_ERR_ARG, "dim_in_0, dim_in_1 and azim_num must be positive");
    if (c.offset_0 < 0 || c.offset_1 < 0 || c.offset_0 + c.dim_in_0 > sc->hdr.d0 || c.offset_1 + c.dim_in_1 > sc->hdr.d1)
        return set_error(HZ_ERR_ARG, "inconsistency between input arguments dem_dim_0, dem_dim_1, offset_0, offset_1 and vec_norm");
    if (!(c.hori_acc > 0.0f) || c.hori_acc > 10.0f) return set_error(HZ_ERR_ARG, "limit of hori_acc (10 degree) is exceeded");
    w->skip_hori = opts && opts->skip_hori;
    w->to_q16 = c.out.hori && (c.out.hori_kind & HZ_HORI_U16);
    w->to_planes = c.out.hori && !w->to_q16 && (c.out.hori_kind & HZ_HORI_PLANES);
    const bool to_layout = w->to_planes || w->to_q16;
    if (to_layout && w->skip_hori)
        return set_error(HZ_ERR_ARG, "skip_hori with %s: there is nothing to lay out", w->to_q16 ? "hori_q" : "hori_planes");
    w->want_dist = c.out.dist != nullptr;
    if (w->want_dist && w->skip_hori) return set_error(HZ_ERR_ARG, "skip_hori with dist_buffer: there is no horizon to return it with");
    if (!c.out.hori && !w->skip_hori) return set_error(HZ_ERR_ARG, "hori_buffer is NULL");
    if (opts && opts->svf && !opts->vec_tilt) return set_error(HZ_ERR_ARG, "opts.svf needs opts.vec_tilt");
    // the SVF weights sectors by azim[1] - azim[0] (topo_param.pyx:433): undefined for a single azimuth
    if (opts && opts->svf && c.azim_num < 2) return set_error(HZ_ERR_ARG, "opts.svf needs azim_num >= 2");
    // further reductions (hz_topo_out): the VSF as the SVF (tilt, azim[1] - azim[0], :520); openness needs neither
    if (topo && topo->size != (int32_t)sizeof(hz_topo_out))
        return set_error(HZ_ERR_ARG, "topo.size is %d, expected sizeof(hz_topo_out) = %d", topo->size, (int)sizeof(hz_topo_out));
    w->want_svf = opts && opts->svf;
    w->want_vsf = topo && topo->vsf; w->want_open = topo && topo->openness;
    if (w->want_vsf && !(opts && opts->vec_tilt)) return set_error(HZ_ERR_ARG, "topo.vsf needs opts.vec_tilt");
    if (w->want_vsf && c.azim_num < 2) return set_error(HZ_ERR_ARG, "topo.vsf needs azim_num >= 2");
    return resolve_row_slab(opts, c.dim_in_0, &w->row_begin, &w->row_end);
}

// Where the chunks of one float32 cell-major quantity (the horizon, the distances) go: `dst` in device or host memory,
// cell-major or planes, float32 or 16-bit codes; the slab's first cell is cell `cell0` of dst (of every plane: plane_stride
// elements apart).  A host destination has a staging buffer of one chunk in the destination's layout -- but for cell-major
// float32, where the chunk itself is what is copied.
struct ChunkSink {
    void *dst = nullptr;
    bool planes = false, q16 = false, on_dev = false;
    size_t plane_stride = 0, cell0 = 0;
    DevBuf staging;
    const char *what = "";               // for the error string
    size_t elem() const { return q16 ? sizeof(uint16_t) : sizeof(float); }
    bool needs_staging() const { return !on_dev && (planes || q16); }
};

// Chunk `chunk` (cc cells from cell c0 of the slab, azim_num values each, on the device) into its place in s.dst, on `st`:
// for a device destination the transposition or the encoder straight into place (cell-major float32: the chunk was
// produced in place, nothing to do), for a host destination the same launch into the staging buffer, `copy_begin` (if given),
// then one copy -- of planes azim_num rows of cc elements, pitch = plane stride.
static int deliver_chunk(const float *chunk, size_t c0, size_t cc, int azim_num, ChunkSink &s, hipStream_t st, Event *copy_begin = nullptr) {
    const size_t A = (size_t)azim_num, cell = s.cell0 + c0, es = s.elem();
    void *lay = s.on_dev ? s.dst : s.staging.p;                                  // where the launch writes ...
    const size_t stride = s.on_dev ? s.plane_stride : cc, first = s.on_dev ? cell : 0;      // ... and its planes there
    int rc = HZ_OK;
    if (s.q16 && s.planes) rc = hori_quantise_planes_launch(chunk, cc, azim_num, static_cast<uint16_t *>(lay), stride, first, st);
    else if (s.q16) rc = hori_quantise_launch(chunk, cc * A, static_cast<uint16_t *>(lay) + first * A, st);
    else if (s.planes) rc = hori_to_planes_launch(chunk, cc, azim_num, static_cast<float *>(lay), stride, first, st);
    if (rc || s.on_dev) return rc;
    if (copy_begin && (rc = copy_begin->record(st))) return rc;
    const void *src = s.needs_staging() ? s.staging.p : chunk;
    char *dst = static_cast<char *>(s.dst);
    const hipError_t ce = s.planes
        ? hipMemcpy2DAsync(dst + cell * es, s.plane_stride * es, src, cc * es, cc * es, A, hipMemcpyDeviceToHost, st)
        : hipMemcpyAsync(dst + cell * A * es, src, cc * A * es, hipMemcpyDeviceToHost, st);
    if (ce != hipSuccess) return set_error(HZ_ERR_HIP, "copy of the %s failed: %s", s.what, hipGetErrorString(ce));
    return HZ_OK;
}

// The events of one chunk: on the kernels' stream, but copy_done (the copy stream of the streamed host output).
struct ChunkEvents {
    Event launch_begin, trace_end, reduce_end, copy_done, followup_begin, codes_copy_begin, codes_copy_end, dist_end, dist_copy_end;
};

// GPU time of a call, interval by interval, and the field of hz_stats each sum is added to (HorizonRun::finish):
//   trace       launch_begin .. trace_end           t_kernel_s  production launch, follow-up launches, redo launches, the monitor
//   followup    followup_begin .. trace_end         t_left_s    (a part of `trace`)
//   reduce      trace_end .. reduce_end             t_svf_s     the SVF / VSF / openness launch
//   dist        reduce_end .. dist_end              t_kernel_s  the distance kernel
//   dist_copy   dist_end .. dist_copy_end           t_d2h_s     the distances into their layout and to a host dist_buffer
//   codes_copy  codes_copy_begin .. codes_copy_end  t_d2h_s     the chunk's codes to a host hori_q
// t_d2h_s also gets the wall time of the copy-out after the last chunk.  The copy of a chunk of planes to a host hori_planes
// lies in no interval: it is counted in t_total_s and nowhere else.
struct ChunkTimes {
    float trace = 0.0f, followup = 0.0f, reduce = 0.0f, dist = 0.0f, dist_copy = 0.0f, codes_copy = 0.0f;      // [ms]
    void add(const ChunkEvents &e) {
        trace += e.launch_begin.ms_until(e.trace_end);
        followup += e.followup_begin.ms_until(e.trace_end);
        reduce += e.trace_end.ms_until(e.reduce_end);
        dist += e.reduce_end.ms_until(e.dist_end);
        dist_copy += e.dist_end.ms_until(e.dist_copy_end);
        codes_copy += e.codes_copy_begin.ms_until(e.codes_copy_end);
    }
};

// The state of one call of horizon_run: set-up, one chunk of rows at a time, read-out.  At the end the copy stream goes back to
// its pool (synchronised); then the members go in reverse order: the pinner (joined, unregistered), the events, the monitor, the buffers.
struct HorizonRun {
    const Scene *sc;
    const HorizonCall &c;
    const HorizonWants &w;
    const hz_opts *opts;
    hipStream_t st, st_copy = nullptr;         // the kernels' stream; the copy stream of the streamed host output
    Timer t_total;
    double h2d_s = 0.0;
    HostTables tb;
    float dist_m = 0.0f;
    size_t slab_cells = 0, row_bytes = 0;
    DevIn<float> d_norm, d_north, d_tilt, d_azim;
    DevIn<uint8_t> d_mask;
    DevTables dt;
    const float *norm0 = nullptr, *north0 = nullptr, *tilt0 = nullptr;      // the inputs as indexed by global cell
    const uint8_t *mask0 = nullptr;
    DevOut<float> d_hori, d_svf, d_vsf, d_open;
    std::vector<float> azim_h;
    bool want_topo = false, stream_out = false, use_near = false, height_field = false, bad_map = false;
    int near_opt = 0, verify_n = 0;
    // rows per launch: the whole slab when `hori` is device memory.  Otherwise the horizon of a chunk of rows lives in a bounded
    // temporary: one <= 4 GiB buffer when only the SVF is wanted, two of them when `hori` is host memory -- chunk c is copied
    // out on a second stream while chunk c + 1 is traced, so the D2H time hides behind the kernel and the output may be larger
    // than HBM.
    int chunk_rows = 0, n_chunk = 0;
    DevBuf tmp_hori, tmp_hori2, tmp_dist;      // chunk buffers of the float32 horizon (two: the streamed host output) and of the cell-major distances
    size_t tmp_bytes = 0;                      // all chunk and staging buffers (hz_stats.scratch_bytes)
    float *hori_slab_host = nullptr, *hori_row0 = nullptr;
    ChunkSink hori_sink, dist_sink;
    DevBuf dist_cnt, cnt_dev, near_reasons;    // [0] distance rays, [1] cells; the counters of HorizonArgs; opts.verbose >= 2: histogram of why cells got no certificate
    unsigned long long zeros[HZ_CNT_N] = {0};  // counters; behind them the lists of tiles to redo (hz_horizon.hip)
    HorizonArgs a;
    int left_t[HZ_LEFT_LEVELS], n_left_launches = 0;
    unsigned long long cnt[16] = {0}, refill_hist[16] = {0};      // sums over the chunks: words 0 .. 15, and counters[HZ_CNT_REFILL ..] of the counting instantiation
    unsigned long long n_verified = 0, n_mon_violations = 0, redo_blocks = 0, redo_groups = 0, left_cells = 0, left_again = 0;
    unsigned long long lend_tests = 0, lend_unhelped = 0;         // counting instantiation with leaf lending (hz_trace)
    int fallbacks = 0;
    float ms_near = 0.0f;
    ChunkTimes times;
    NearMonitor mon;
    std::vector<ChunkEvents> evs;              // one per chunk
    HostPinner pinner;

    HorizonRun(const Scene *sc_, const HorizonCall &c_, const HorizonWants &w_) : sc(sc_), c(c_), w(w_), opts(c_.opts), st(sc_->stream) {}
    ~HorizonRun() { if (st_copy) stream_release(sc->device, st_copy); }
    int setup();
    int setup_outputs();
    int copy_out(int k);
    int launch_chunk(int *safe_out);
    int trace_chunk(int rb, int re);
    int chunk(int rb);
    int distances(const float *hori_chunk, int rb, int re, ChunkEvents &e);
    int fail(int code) { (void)hipStreamSynchronize(st); if (st_copy) (void)hipStreamSynchronize(st_copy); return code; }
    int finish();
};

// uploads, tables, HorizonArgs
int HorizonRun::setup() {
    int rc;
    t_total.start();
    const int dim_in_1 = c.dim_in_1, azim_num = c.azim_num, row_begin = w.row_begin;
    // unit conversions: horizon_comp.cpp:667-670
    build_tables(azim_num, c.hori_acc, c.elev_ang_low_lim, tb);
    if (tb.elev_num < 2) return set_error(HZ_ERR_ARG, "elevation table is empty (elev_ang_low_lim too high)");
    dist_m = (float)((double)c.dist_search * 1000.0);
    slab_cells = (size_t)(w.row_end - row_begin) * dim_in_1;
    row_bytes = (size_t)dim_in_1 * azim_num * 4;
    Timer t_h2d; t_h2d.start();
    // Per-cell inputs: only the slab's rows are ever read, so only those are uploaded when the arrays are host memory.
    // opts.inputs_are_slab: the four pointers address row_begin (a rank of a sharded job holds -- and uploads -- its own
    // rows only); otherwise they address inner-domain row 0 (the reference's layout).  The kernels index by global
    // cell: `in_off` shifts the slab-local device addresses back (address arithmetic only, never dereferenced outside
    // the slab).
    const size_t in_off = (size_t)row_begin * dim_in_1;
    const size_t src_off = (opts && opts->inputs_are_slab) ? 0 : in_off;
    if ((rc = d_norm.bind(c.vec_norm + 3 * src_off, slab_cells * 3, st))) return rc;
    if ((rc = d_north.bind(c.vec_north + 3 * src_off, slab_cells * 3, st))) return rc;
    if ((rc = d_mask.bind(c.mask + src_off, slab_cells, st))) return rc;
    if (w.want_svf || w.want_vsf) if ((rc = d_tilt.bind(opts->vec_tilt + 3 * src_off, slab_cells * 3, st))) return rc;
    norm0 = d_norm.dev - 3 * in_off; north0 = d_north.dev - 3 * in_off;
    mask0 = d_mask.dev - in_off;
    tilt0 = d_tilt.dev ? d_tilt.dev - 3 * in_off : nullptr;
    if ((rc = dt.bind(tb, true, st))) return rc;
    want_topo = w.want_svf || w.want_vsf || w.want_open;
    if ((rc = setup_outputs())) return rc;
    if (want_topo) {   // azim as the wrapper recomputes it, horizon.pyx:191-195
        azim_h.resize((size_t)azim_num);
        for (int i = 0; i < azim_num; i++) azim_h[(size_t)i] = (float)(((2 * M_PI) / azim_num) * i);
        if ((rc = d_azim.bind(azim_h.data(), (size_t)azim_num, st))) return rc;
    }
    HZ_HIP(cnt_dev.alloc(sizeof(zeros) + 2 * HZ_REDO_CAP * sizeof(int)));      // (two lists: blocks, and groups of the leftover launch)
    HZ_HIP(hipStreamSynchronize(st));
    h2d_s = t_h2d.stop();

    a.vec_norm = norm0; a.vec_north = north0; a.mask = mask0;
    a.offset_0 = c.offset_0; a.offset_1 = c.offset_1; a.dim_in_0 = c.dim_in_0; a.dim_in_1 = dim_in_1;
    a.azim_num = azim_num; a.elev_num = tb.elev_num; a.alg = w.alg;
    a.hori_acc = tb.hori_acc; a.low = tb.low; a.up = tb.up; a.dist = dist_m;
    a.hori_fill = c.hori_fill; a.ray_org_elev = c.ray_org_elev;
    a.azim_sin = dt.azim_sin.dev; a.azim_cos = dt.azim_cos.dev; a.elev_ang = dt.elev_ang.dev; a.elev_sin = dt.elev_sin.dev; a.elev_cos = dt.elev_cos.dev;
    a.mid_idx = dt.mid_idx.dev;
    a.top_nodes = opts ? opts->top_nodes : -1;
    a.regroup = opts ? opts->regroup : -1;
    a.count_work = opts ? opts->count_work : 0;
    a.hit_cache = (opts && opts->no_hit_cache) ? 0 : 1;
    a.counters = static_cast<unsigned long long *>(cnt_dev.p);
    // near-field certificates (hz_near.hip): one pre-pass per chunk into a scratch buffer kept with the scene.
    // Off beyond the azimuth count the pre-pass holds in LDS, and on request.  The distance bound near_r assumes a height
    // field over the world (x, y) plane (HZ_BLOB_HEIGHT_FIELD, checked by the scene build).  Where only SOME quads break
    // that, or an outer-domain TIN is present, the scene carries a bitmap of their (x, y) footprints (HZ_BLOB_BAD_MAP) and
    // the pre-pass refuses the cells near them, one by one (round 5; rounds 3-4: off for the whole scene).  Neither flag
    // (a bad primitive too large to rasterise): off.  opts.no_near_skip < 0 overrides both checks (tests only).
    near_opt = opts ? opts->no_near_skip : 0;
    height_field = (sc->hdr.flags & HZ_BLOB_HEIGHT_FIELD) != 0;
    bad_map = (sc->hdr.flags & HZ_BLOB_BAD_MAP) != 0;
    use_near = near_opt <= 0 && (height_field || bad_map || near_opt < 0) && azim_num <= near_max_azim() && tb.elev_num <= 65534;
    a.near_idx = nullptr; a.near_r = nullptr; a.scratch_row = nullptr;
    a.tile_list = nullptr; a.n_list = 0;
    // opts.verify_near = N: with count_work the counting instantiation re-traces one of every N shortened rays; without it
    // the production launch stays as it is and a second, counting launch re-traces EVERY shortened ray of one of every N
    // 8 x 8 blocks (the monitor for production inputs)
    verify_n = (opts && opts->verify_near > 0) ? opts->verify_near : 0;
    a.verify_near = (opts && opts->count_work) ? verify_n : 0;

    if (stream_out && (rc = stream_acquire(sc->device, &st_copy))) return rc;
    const int rows_max = std::min(chunk_rows, w.row_end - row_begin);
    // the certificate scratch of the largest chunk, allocated before the pinner thread starts (page locking and hipMalloc
    // serialise in the driver)
    if (use_near && (rc = grow_near_scratch(sc, (size_t)rows_max * dim_in_1, azim_num))) return rc;
    n_left_launches = plan_leftover(sc, opts, rows_max, dim_in_1, left_t, a);
    a.left_min = n_left_launches > 0 ? left_t[0] : 0;
    a.left_rec = n_left_launches > 0 ? (unsigned *)sc->left_buf : nullptr;
    a.left_regroup = (opts && (opts->left_tune & 0xff) > 0) ? (opts->left_tune & 0xff) : (regroup_rule_of(a.regroup) ? HZ_LEFT_REGROUP_REL : HZ_LEFT_REGROUP);
    a.left_key_shift = (opts && ((opts->left_tune >> 8) & 0xff) > 0) ? std::min(((opts->left_tune >> 8) & 0xff) - 1, 8) : HZ_LEFT_KEY_SHIFT;
    a.persist_grid = (opts && opts->persist_grid > 0) ? opts->persist_grid : 0;
    a.no_persist = (opts && opts->persist_grid < 0) ? 1 : 0;
    if (use_near && opts && opts->verbose >= 2) {      // printed to stderr at the end of the call
        if (near_reasons.alloc(20 * sizeof(unsigned)) != hipSuccess) { (void)hipGetLastError(); near_reasons.p = nullptr; }
        else (void)hipMemsetAsync(near_reasons.p, 0, 20 * sizeof(unsigned), st);
    }
    if (stream_out && !(opts && opts->no_host_pin)) {
        std::vector<size_t> cb;
        for (int rb = row_begin; rb < w.row_end; rb += chunk_rows) cb.push_back((size_t)(std::min(rb + chunk_rows, w.row_end) - rb) * row_bytes);
        pinner.start(sc->device, reinterpret_cast<char *>(hori_slab_host), cb);
    }
    return HZ_OK;
}

// the maps, the horizon's and the distances' sinks, the chunk and staging buffers
int HorizonRun::setup_outputs() {
    int rc;
    const int dim_in_1 = c.dim_in_1, azim_num = c.azim_num, row_begin = w.row_begin, rows = w.row_end - w.row_begin;
    const hz_topo_out *topo = c.topo;
    // hori_buffer addresses inner-domain row 0 (the reference's layout) unless opts.hori_is_slab says it addresses
    // row_begin.  Only the slab itself is ever classified or written: `hori_row0` is an address used for
    // arithmetic alone (it may lie below the caller's allocation when a resident slab buffer is passed).
    const bool hori_is_slab = opts && opts->hori_is_slab;
    const bool to_layout = w.to_planes || w.to_q16;
    float *hori_buffer = to_layout ? nullptr : static_cast<float *>(c.out.hori);
    hori_slab_host = hori_buffer ? (hori_is_slab ? hori_buffer : hori_buffer + (size_t)row_begin * dim_in_1 * azim_num) : nullptr;
    hori_row0 = hori_slab_host ? hori_slab_host - (size_t)row_begin * dim_in_1 * azim_num : nullptr;
    // opts.svf and the maps of hz_topo_out address row 0 or row_begin exactly as hori_buffer does
    const size_t map_off = hori_is_slab ? 0 : (size_t)row_begin * dim_in_1;
    float *svf_slab = w.want_svf ? opts->svf + map_off : nullptr;
    float *vsf_slab = w.want_vsf ? topo->vsf + map_off : nullptr;
    float *open_slab = w.want_open ? topo->openness + map_off : nullptr;
    if ((rc = d_svf.bind(svf_slab, svf_slab ? slab_cells : 0))) return rc;
    if ((rc = d_vsf.bind(vsf_slab, vsf_slab ? slab_cells : 0))) return rc;
    if ((rc = d_open.bind(open_slab, open_slab ? slab_cells : 0))) return rc;
    // planes: stride of one plane and the plane element of the slab's first cell, by the rules of hori_buffer
    const size_t plane_stride = hori_is_slab ? slab_cells : (size_t)c.dim_in_0 * dim_in_1;
    hori_sink.dst = to_layout ? c.out.hori : nullptr;
    hori_sink.planes = w.to_planes || (w.to_q16 && (c.out.hori_kind & HZ_HORI_PLANES)); hori_sink.q16 = w.to_q16;
    hori_sink.on_dev = to_layout && is_device_ptr(c.out.hori);
    hori_sink.plane_stride = plane_stride; hori_sink.cell0 = map_off;
    hori_sink.what = w.to_q16 ? "horizon codes" : "horizon planes";
    chunk_rows = rows;
    stream_out = !w.skip_hori && !to_layout && !is_device_ptr(hori_slab_host);
    if (w.skip_hori || to_layout || stream_out) {
        if (w.skip_hori && !want_topo) return set_error(HZ_ERR_ARG, "skip_hori without svf, vsf or openness: nothing to compute");
        if ((rc = alloc_hori_chunk(rows, row_bytes, w.skip_hori, (opts && opts->chunk_rows > 0) ? opts->chunk_rows : 0, &chunk_rows, &tmp_hori)))
            return rc;
        const size_t chunk_bytes = (size_t)chunk_rows * row_bytes;
        tmp_bytes = chunk_bytes;
        if (stream_out && chunk_rows < rows) { HZ_HIP(tmp_hori2.alloc(chunk_bytes)); tmp_bytes += chunk_bytes; }
        if (to_layout && hori_sink.needs_staging()) {
            const size_t bytes = chunk_bytes / sizeof(float) * hori_sink.elem();
            HZ_HIP(hori_sink.staging.alloc(bytes)); tmp_bytes += bytes;
        }
    } else {
        if ((rc = d_hori.bind(hori_slab_host, slab_cells * (size_t)azim_num))) return rc;
    }
    // the distances of a chunk: cell-major in a chunk buffer unless dist_buffer is device memory in that layout; planes reach
    // a device dist_buffer through the transposition of hori_planes, a host one through one more chunk buffer
    if (w.want_dist) {
        const size_t chunk_bytes = (size_t)chunk_rows * row_bytes;
        dist_sink.dst = c.out.dist;
        dist_sink.planes = (c.out.hori_kind & HZ_HORI_PLANES) != 0;
        dist_sink.on_dev = is_device_ptr(c.out.dist);
        dist_sink.plane_stride = plane_stride; dist_sink.cell0 = map_off;
        dist_sink.what = dist_sink.planes ? "distance planes" : "distances";
        if (!dist_sink.on_dev || dist_sink.planes) { HZ_HIP(tmp_dist.alloc(chunk_bytes)); tmp_bytes += chunk_bytes; }
        if (dist_sink.needs_staging()) { HZ_HIP(dist_sink.staging.alloc(chunk_bytes)); tmp_bytes += chunk_bytes; }
        HZ_HIP(dist_cnt.alloc(2 * sizeof(unsigned long long)));
        HZ_HIP(hipMemsetAsync(dist_cnt.p, 0, 2 * sizeof(unsigned long long), st));
    }
    return HZ_OK;
}

// copy of chunk k of the streamed host output (issued after chunk k + 1 was launched, so a host-blocking pageable copy still overlaps)
int HorizonRun::copy_out(int k) {
    const int rb = w.row_begin + k * chunk_rows, re = std::min(rb + chunk_rows, w.row_end);
    const void *src = (k & 1) ? tmp_hori2.p : tmp_hori.p;
    ChunkEvents &e = evs[(size_t)k];
    char *dst = reinterpret_cast<char *>(hori_row0 + (size_t)rb * c.dim_in_1 * c.azim_num);
    const size_t bytes = (size_t)(re - rb) * row_bytes;
    // a copy must not straddle two separately page-locked ranges (nor a locked and a pageable one): cut it at every
    // region boundary inside the chunk (at most three pieces; the slab's unaligned head and tail stay pageable)
    std::vector<size_t> cuts;
    if (!pinner.planned.empty()) cuts = pinner.cuts_for(dst, bytes);
    cuts.push_back(bytes);
    if (hipStreamWaitEvent(st_copy, e.reduce_end.e, 0) != hipSuccess)
        return set_error(HZ_ERR_HIP, "copy of the horizon chunk failed: %s", hipGetErrorString(hipGetLastError()));
    size_t from = 0;
    for (size_t to : cuts) {
        if (to > from && hipMemcpyAsync(dst + from, static_cast<const char *>(src) + from, to - from, hipMemcpyDeviceToHost, st_copy) != hipSuccess)
            return set_error(HZ_ERR_HIP, "copy of the horizon chunk failed: %s", hipGetErrorString(hipGetLastError()));
        from = to;
    }
    if (e.copy_done.record(st_copy))
        return set_error(HZ_ERR_HIP, "copy of the horizon chunk failed: %s", hipGetErrorString(hipGetLastError()));
    return HZ_OK;
}

// production launch + the follow-up launches of the cells it leaves unfinished (no host wait in between)
int HorizonRun::launch_chunk(int *safe_out) {
    int r = horizon_launch(sc, a, st, safe_out);
    if (r || n_left_launches == 0) return r;
    if ((r = evs.back().followup_begin.record(st))) return r;
    for (int l = 1; l <= n_left_launches && !r; l++) {
        if ((r = left_sort(a, l - 1, st))) break;
        HorizonArgs b = a;
        b.left_mode = l; b.left_min = l < n_left_launches ? left_t[l] : 0;
        // a single follow-up launch runs the stack discipline of the production launch (a group whose fast stack overflows is
        // computed again, below, from the sorted order this launch used); with several levels they run one entry per level:
        // nothing can overflow there (and the next level's sort reuses the buffers of this one's)
        if (n_left_launches > 1) b.level_stack = 1;
        b.tile_list = nullptr; b.n_list = 0;
        r = horizon_launch(sc, b, st, nullptr);
    }
    return r;
}

// Rows [rb, re) into a.hori: counter reset, launch_begin, the monitor, the launches, and -- fast stack discipline -- the
// blocks that ran out of entries again; the monitor's tallies.  HIP failures of its own go through fail().
int HorizonRun::trace_chunk(int rb, int re) {
    int rc;
    ChunkEvents &e = evs.back();
    if (hipMemcpyAsync(cnt_dev.p, zeros, sizeof(zeros), hipMemcpyHostToDevice, st) != hipSuccess)
        return set_error(HZ_ERR_HIP, "counter reset failed");
    // the buffer of chunk n is the one chunk n - 2 was copied out of
    if (stream_out && n_chunk >= 2) (void)hipStreamWaitEvent(st, evs[(size_t)n_chunk - 2].copy_done.e, 0);
    a.level_stack = (sc->level_stack.load(std::memory_order_relaxed) != 0 || (opts && opts->level_stack > 0)) ? 1
                    : ((opts && opts->level_stack < 0) ? opts->level_stack : 0);
    if ((rc = e.launch_begin.record(st))) return rc;
    if (verify_n > 0 && !a.count_work && use_near) {
        // monitor: the certificates of a sample of this launch's blocks, checked ray by ray by a counting launch
        // (every shortened ray traced a second time over its full length) on a stream of its own, so that its few
        // workgroups run NEXT TO the production launch instead of after it (a launch of its own costs one
        // workgroup lifetime, ~0.1 s, however small the sample).  Its stores go to a scratch row (HorizonArgs::scratch_row).
        if ((rc = mon.launch(sc, a, verify_n, rb, st))) return rc;
    }
    int safe = 0;
    rc = launch_chunk(&safe);
    if (!rc && !safe) {
        // fast stack discipline: did a wave run out of entries?  Its 8 x 8 block does not count (and handed nothing over) and is
        // computed again with the one-entry-per-level kernel: block by block when they are few (deep trees overflow in a
        // few places only), the whole launch -- and every later launch on this scene -- when they are many
        unsigned long long cov[32] = {0};
        if (hipMemcpyAsync(cov, cnt_dev.p, sizeof(cov), hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipStreamSynchronize(st) != hipSuccess)
            return set_error(HZ_ERR_HIP, "horizon kernel failed: %s", hipGetErrorString(hipGetLastError()));
        const unsigned long long ov = cov[HZ_CNT_OVERFLOW], lov = cov[HZ_CNT_LEFT_OVERFLOW];
        if (ov != 0 || lov != 0) {
            const unsigned long long tiles = (unsigned long long)((re - rb + 7) / 8) * (unsigned long long)((c.dim_in_1 + 7) / 8);   // 8 x 8 blocks
            const int *redo_list = reinterpret_cast<const int *>(static_cast<unsigned long long *>(cnt_dev.p) + HZ_CNT_N);
            fallbacks++;
            a.level_stack = 1;
            if (ov <= HZ_REDO_CAP && lov <= HZ_REDO_CAP && (ov + lov) * 4 <= tiles) {
                redo_blocks += ov + lov; redo_groups += lov;
                if (ov != 0) {
                    a.tile_list = redo_list;
                    a.n_list = (int)ov;
                    rc = horizon_launch(sc, a, st, &safe);
                    a.tile_list = nullptr; a.n_list = 0;
                }
                if (!rc && lov != 0) {
                    HorizonArgs b = a;
                    b.left_mode = 1; b.left_min = 0;
                    b.tile_list = redo_list + HZ_REDO_CAP;
                    b.n_list = (int)lov;
                    rc = horizon_launch(sc, b, st, nullptr);
                }
            } else {
                sc->level_stack.store(1, std::memory_order_relaxed);
                if (hipMemcpyAsync(cnt_dev.p, zeros, sizeof(zeros), hipMemcpyHostToDevice, st) != hipSuccess)
                    return set_error(HZ_ERR_HIP, "counter reset failed");
                if ((rc = e.launch_begin.record(st))) return rc;
                rc = launch_chunk(&safe);
            }
        }
    }
    if (!rc && mon.active) rc = mon.collect(st, &n_verified, &n_mon_violations);
    return rc;
}

// the distances of rows [rb, re) from their float32 horizon, before that is laid out or encoded
int HorizonRun::distances(const float *hori_chunk, int rb, int re, ChunkEvents &e) {
    const size_t cc = (size_t)(re - rb) * c.dim_in_1, c0 = (size_t)(rb - w.row_begin) * c.dim_in_1;
    float *dist_chunk = tmp_dist.p ? static_cast<float *>(tmp_dist.p) : c.out.dist + (dist_sink.cell0 + c0) * (size_t)c.azim_num;
    HoridistArgs da;
    da.vec_norm = norm0; da.vec_north = north0; da.mask = mask0;
    da.hori = hori_chunk; da.dist = dist_chunk; da.q16 = 0; da.planes = 0;
    da.hori_stride = da.hori_cell0 = da.dist_stride = da.dist_cell0 = 0;
    da.offset_0 = c.offset_0; da.offset_1 = c.offset_1; da.dim_in_1 = c.dim_in_1; da.row_begin = rb; da.row_end = re;
    da.azim_num = c.azim_num; da.elev_num = tb.elev_num;
    da.hori_acc = tb.hori_acc; da.up = tb.up; da.dist_m = dist_m; da.ray_org_elev = c.ray_org_elev;
    da.azim_sin = dt.azim_sin.dev; da.azim_cos = dt.azim_cos.dev; da.elev_ang = dt.elev_ang.dev; da.elev_sin = dt.elev_sin.dev; da.elev_cos = dt.elev_cos.dev;
    da.block_w = 8; da.counters = static_cast<unsigned long long *>(dist_cnt.p);
    int rc = horidist_launch(sc, da, st);
    const int rc_ev = e.dist_end.record(st);
    if (!rc && !rc_ev) rc = deliver_chunk(dist_chunk, c0, cc, c.azim_num, dist_sink, st);
    const int rc_ev2 = e.dist_copy_end.record(st);
    return rc ? rc : (rc_ev ? rc_ev : rc_ev2);
}

// one chunk of rows from row rb: certificates, trace, reduce, distances, delivery, the counters' read-out
int HorizonRun::chunk(int rb) {
    int rc;
    const int re = std::min(rb + chunk_rows, w.row_end), dim_in_1 = c.dim_in_1, azim_num = c.azim_num;
    const bool to_layout = w.to_planes || w.to_q16;
    // the kernels index hori by global cell: shift the (slab- or chunk-local) buffer back
    float *hori_chunk;
    if (stream_out) hori_chunk = static_cast<float *>((n_chunk & 1) ? tmp_hori2.p : tmp_hori.p);
    else if (w.skip_hori || to_layout) hori_chunk = static_cast<float *>(tmp_hori.p);
    else hori_chunk = d_hori.dev + (size_t)(rb - w.row_begin) * dim_in_1 * azim_num;
    a.hori = hori_chunk - (size_t)rb * dim_in_1 * azim_num;
    a.row_begin = rb; a.row_end = re;
    if (use_near) {
        NearArgs na;
        na.vec_norm = norm0; na.vec_north = north0; na.mask = mask0;
        na.azim_sin = dt.azim_sin.dev; na.azim_cos = dt.azim_cos.dev;
        na.offset_0 = c.offset_0; na.offset_1 = c.offset_1; na.dim_in_1 = dim_in_1; na.row_begin = rb; na.row_end = re;
        na.azim_num = azim_num; na.elev_num = tb.elev_num;
        na.ray_org_elev = c.ray_org_elev; na.hori_acc = tb.hori_acc; na.low = tb.low; na.up = tb.up;
        na.reasons = static_cast<unsigned *>(near_reasons.p);
        na.ignore_bad_map = near_opt < 0 ? 1 : 0;
        if ((rc = near_prepass(sc, na, st, &ms_near))) return rc;
        a.near_idx = na.near_idx; a.near_r = na.near_r;
    }
    evs.emplace_back();
    ChunkEvents &e = evs.back();
    rc = trace_chunk(rb, re);
    const int rc_b = e.trace_end.record(st);
    if (!rc) rc = rc_b;
    if (!rc && want_topo) {
        // one reduction launch per chunk, whatever the maps (the SVF alone is k_topo<1>)
        const size_t o = (size_t)(rb - w.row_begin) * dim_in_1;
        const float *tilt_chunk = tilt0 ? tilt0 + 3 * (size_t)rb * dim_in_1 : nullptr;
        rc = topo_launch(d_azim.dev, hori_chunk, tilt_chunk, re - rb, dim_in_1, azim_num,
                         w.want_svf ? d_svf.dev + o : nullptr, w.want_vsf ? d_vsf.dev + o : nullptr,
                         w.want_open ? d_open.dev + o : nullptr, st);
    }
    const int rc_c = e.reduce_end.record(st);
    if (!rc) rc = rc_c;
    if (!rc && w.want_dist) rc = distances(hori_chunk, rb, re, e);
    if (!rc && to_layout) {
        // the chunk into its rows of every plane, or as codes into its place
        const bool timed = w.to_q16 && !hori_sink.on_dev;      // (see ChunkTimes: the copy of planes is not)
        rc = deliver_chunk(hori_chunk, (size_t)(rb - w.row_begin) * dim_in_1, (size_t)(re - rb) * dim_in_1, azim_num, hori_sink, st,
                           timed ? &e.codes_copy_begin : nullptr);
        if (timed && e.codes_copy_begin.e) { const int rc_r = e.codes_copy_end.record(st); if (!rc) rc = rc_r; }
    }
    if (!rc && stream_out && n_chunk >= 1) rc = copy_out(n_chunk - 1);
    if (rc) return rc;
    unsigned long long cw[HZ_CNT_N];
    if (hipMemcpyAsync(cw, cnt_dev.p, sizeof(cw), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
        return set_error(HZ_ERR_HIP, "horizon kernel failed: %s", hipGetErrorString(hipGetLastError()));
    times.add(e);
    for (int k = 0; k < 16; k++) cnt[k] += cw[k];
    left_cells += cw[HZ_CNT_LEFT_CELLS]; left_again += cw[HZ_CNT_LEFT_AGAIN];
    n_verified += cw[HZ_CNT_VERIFIED];
    lend_tests += cw[HZ_CNT_LENT]; lend_unhelped += cw[HZ_CNT_UNHELPED];
    for (int k = 0; k < 16; k++) refill_hist[k] += cw[HZ_CNT_REFILL + k];
    if (a.count_work && opts && opts->verbose >= 3) {      // per-XCD span of this launch (counting instantiation)
        const unsigned long long t0 = ~cw[HZ_CNT_START];
        fprintf(stderr, "hz xcd spans [ms] rows %d..%d:", rb, re);
        for (int x = 0; x < 8; x++) fprintf(stderr, " %.1f", cw[HZ_CNT_XCD_END + x] ? (double)(cw[HZ_CNT_XCD_END + x] - t0) * 1.0e-5 : 0.0);
        fprintf(stderr, "\n");
    }
    n_chunk++;
    return HZ_OK;
}

// the last copy-out, the maps, hz_stats, the reports
int HorizonRun::finish() {
    int rc = HZ_OK;
    Timer t_d2h; t_d2h.start();
    if (stream_out) {
        rc = copy_out(n_chunk - 1);
        const hipError_t se = hipStreamSynchronize(st_copy);
        pinner.finish();
        if (!rc && se != hipSuccess) rc = set_error(HZ_ERR_HIP, "copy of the horizon failed: %s", hipGetErrorString(se));
        if (rc) return rc;
    }
    HZ_HIP(hipGetLastError());
    if ((rc = d_hori.finish(st))) return rc;
    if ((rc = d_svf.finish(st))) return rc;
    if ((rc = d_vsf.finish(st))) return rc;
    if ((rc = d_open.finish(st))) return rc;
    HZ_HIP(hipStreamSynchronize(st));
    const double d2h_s = t_d2h.stop();
    unsigned long long dcnt[2] = {0, 0};
    if (w.want_dist) HZ_HIP(hipMemcpy(dcnt, dist_cnt.p, sizeof(dcnt), hipMemcpyDeviceToHost));
    if (hz_stats *stats = c.stats) {
        // (the intervals: ChunkTimes.  A call with dist_buffer: the distance rays count as rays)
        stats->num_rays += dcnt[0] + cnt[HZ_CNT_RAYS]; stats->guard_events += cnt[HZ_CNT_GUARDS];
        stats->nodes_visited += cnt[HZ_CNT_NODES]; stats->tris_tested += cnt[HZ_CNT_TRIS]; stats->num_cells += cnt[HZ_CNT_CELLS];
        stats->wave_node_iters += cnt[HZ_CNT_WAVE_NODE]; stats->wave_leaf_iters += cnt[HZ_CNT_WAVE_LEAF]; stats->wave_refills += cnt[HZ_CNT_WAVE_REFILL];
        stats->t_kernel_s += (double)times.dist * 1e-3; stats->t_kernel_s += (double)times.trace * 1e-3;
        stats->t_svf_s += (double)times.reduce * 1e-3;
        stats->t_left_s += (double)times.followup * 1e-3;
        stats->t_d2h_s += (double)times.dist_copy * 1e-3; stats->t_d2h_s += d2h_s + (double)times.codes_copy * 1e-3;
        stats->t_h2d_s += h2d_s; stats->t_near_s += (double)ms_near * 1e-3;
        stats->t_total_s += t_total.stop();
        stats->elev_num = tb.elev_num; stats->bvh_height = sc->hdr.height; stats->scene_bytes = sc->hdr.total_bytes;
        stats->stack_fallbacks += (uint64_t)fallbacks; stats->stack_redo_blocks += redo_blocks; stats->left_redo_groups += redo_groups;
        stats->rays_shortened += cnt[HZ_CNT_SHORTENED]; stats->near_violations += cnt[HZ_CNT_VIOLATIONS] + n_mon_violations;
        stats->guard_cells += cnt[HZ_CNT_GUARD_CELLS]; stats->near_verified += n_verified;
        stats->left_cells += left_cells; stats->left_again += left_again;
        stats->scratch_bytes = (uint64_t)((use_near ? sc->near_bytes : 0) + (n_left_launches > 0 ? sc->left_bytes : 0) + tmp_bytes);
        stats->height_field = height_field ? 1 : 0; stats->near_used = use_near ? 1 : 0;
    }
    // what opts.verbose asks for: diagnostics to stderr, the reference's report to stdout
    if (near_reasons.p) print_near_reasons(static_cast<const unsigned *>(near_reasons.p));
    if (a.count_work && opts && opts->verbose >= 2 && lend_tests + lend_unhelped > 0)      // (a launch with leaf lending ran)
        fprintf(stderr, "hz leaf lending: %llu lent leaf tests, %llu leaf-step lanes with a second leaf and no helper (a = %.3f); "
                        "wave leaf steps %llu, wave node steps %llu, triangles tested %llu\n", lend_tests, lend_unhelped,
                (lend_tests + lend_unhelped) ? (double)lend_tests / (double)(lend_tests + lend_unhelped) : 0.0,
                cnt[HZ_CNT_WAVE_LEAF], cnt[HZ_CNT_WAVE_NODE], cnt[HZ_CNT_TRIS]);
    if (a.count_work && opts && opts->verbose >= 2) {
        // refills of the counting instantiation by population (8 buckets of 8 lanes): how many lanes a refill serves, and how
        // many enter the traversal behind it
        fprintf(stderr, "hz refills (regroup rule %d) by lanes served  1-8 .. 57-64:", regroup_rule_of(a.regroup));
        for (int k = 0; k < 8; k++) fprintf(stderr, " %llu", refill_hist[k]);
        fprintf(stderr, "\nhz refills by lanes entering the traversal 1-8 .. 57-64:");
        for (int k = 8; k < 16; k++) fprintf(stderr, " %llu", refill_hist[k]);
        fprintf(stderr, "\n");
    }
    if (opts && opts->verbose)
        print_reference_report(sc, w.alg, cnt[HZ_CNT_CELLS], cnt[HZ_CNT_RAYS], slab_cells, c.dim_in_0, c.dim_in_1, c.azim_num, (double)times.trace * 1e-3,
                               !use_near && near_opt <= 0 && !height_field && !bad_map, use_near && bad_map);
    return HZ_OK;
}

static int horizon_run(const Scene *sc, const HorizonCall &c) {
    HorizonWants w;
    int rc = check_horizon_call(sc, c, &w);
    if (rc || w.row_begin == w.row_end) return rc;
    HZ_HIP(hipSetDevice(sc->device));
    std::lock_guard<std::mutex> run_lock(sc->run_mu);     // one call at a time on a scene's stream and scratch
    HorizonRun run(sc, c, w);
    if ((rc = run.setup())) return rc;
    for (int rb = w.row_begin; rb < w.row_end; rb += run.chunk_rows)
        if ((rc = run.chunk(rb))) return run.fail(rc);
    return run.finish();
}

static int locations_run(const Scene *sc, const float *coords, const float *vec_norm, const float *vec_north,
                         float *hori_buffer, float *hori_dist_buffer, int num_loc, int azim_num,
                         float dist_search, float hori_acc, const char *ray_algorithm, float elev_ang_low_lim,
                         const float *ray_org_elev, int hori_dist_out, const hz_opts *opts, hz_stats *stats) {
    int alg = 1;
    int rc = parse_alg(ray_algorithm, &alg);
    if (rc) return rc;
    if (hori_dist_out && alg == 2)
        return set_error(HZ_ERR_ARG, "horizon detection algorithm 'guess_constant' not implemented for horizon "
                                     "distance computation");
    if (!coords || !vec_norm || !vec_north || !ray_org_elev || !hori_buffer) return set_error(HZ_ERR_ARG, "NULL argument");
    if (hori_dist_out && !hori_dist_buffer) return set_error(HZ_ERR_ARG, "hori_dist_buffer is NULL");
    if (num_loc <= 0 || azim_num <= 0) return set_error(HZ_ERR_ARG, "num_loc and azim_num must be positive");
    if (!(hori_acc > 0.0f) || hori_acc > 10.0f) return set_error(HZ_ERR_ARG, "limit of hori_acc (10 degree) is exceeded");
    HZ_HIP(hipSetDevice(sc->device));
    std::lock_guard<std::mutex> run_lock(sc->run_mu);
    hipStream_t st = sc->stream;
    Timer t_total; t_total.start();
    HostTables tb;
    build_tables(azim_num, hori_acc, elev_ang_low_lim, tb);
    if (tb.elev_num < 2) return set_error(HZ_ERR_ARG, "elevation table is empty (elev_ang_low_lim too high)");
    Timer t_h2d; t_h2d.start();
    DevIn<float> d_co, d_norm, d_north, d_roe;
    DevTables dt;
    const size_t n = (size_t)num_loc;
    if ((rc = d_co.bind(coords, n * 3, st))) return rc;
    if ((rc = d_norm.bind(vec_norm, n * 3, st))) return rc;
    if ((rc = d_north.bind(vec_north, n * 3, st))) return rc;
    if ((rc = d_roe.bind(ray_org_elev, n, st))) return rc;
    if ((rc = dt.bind(tb, true, st))) return rc;
    // outputs are read-modify-write (untouched rows keep the caller's NaN): copy them in first
    DevOut<float> d_hori, d_dist;
    if ((rc = d_hori.bind(hori_buffer, n * (size_t)azim_num))) return rc;
    if (d_hori.host) HZ_HIP(hipMemcpyAsync(d_hori.dev, hori_buffer, n * (size_t)azim_num * 4, hipMemcpyHostToDevice, st));
    if (hori_dist_out) {
        if ((rc = d_dist.bind(hori_dist_buffer, n * (size_t)azim_num))) return rc;
        if (d_dist.host) HZ_HIP(hipMemcpyAsync(d_dist.dev, hori_dist_buffer, n * (size_t)azim_num * 4, hipMemcpyHostToDevice, st));
    }
    DevBuf cnt_dev;
    unsigned long long zeros[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    HZ_HIP(cnt_dev.alloc(sizeof(zeros)));
    HZ_HIP(hipMemcpyAsync(cnt_dev.p, zeros, sizeof(zeros), hipMemcpyHostToDevice, st));
    HZ_HIP(hipStreamSynchronize(st));
    const double h2d_s = t_h2d.stop();

    LocationsArgs a;
    a.coords = d_co.dev; a.vec_norm = d_norm.dev; a.vec_north = d_north.dev; a.ray_org_elev = d_roe.dev;
    a.hori = d_hori.dev; a.dist = d_dist.dev;
    a.num_loc = num_loc; a.azim_num = azim_num; a.elev_num = tb.elev_num; a.alg = alg; a.hori_dist_out = hori_dist_out;
    a.hori_acc = tb.hori_acc; a.low = tb.low; a.up = tb.up; a.dist_m = (float)((double)dist_search * 1000.0);
    a.azim_sin = dt.azim_sin.dev; a.azim_cos = dt.azim_cos.dev; a.elev_ang = dt.elev_ang.dev; a.elev_sin = dt.elev_sin.dev; a.elev_cos = dt.elev_cos.dev;
    a.mid_idx = dt.mid_idx.dev;
    a.counters = static_cast<unsigned long long *>(cnt_dev.p);
    Event e0, e1;
    if ((rc = e0.record(st))) return rc;
    rc = locations_launch(sc, a, st);
    const int rc_e1 = e1.record(st);
    const hipError_t se = hipStreamSynchronize(st);
    const float ms = e0.ms_until(e1);
    if (rc || rc_e1) return rc ? rc : rc_e1;
    if (se != hipSuccess) return set_error(HZ_ERR_HIP, "locations kernel failed: %s", hipGetErrorString(se));
    Timer t_d2h; t_d2h.start();
    unsigned long long cnt[8];
    HZ_HIP(hipMemcpyAsync(cnt, cnt_dev.p, sizeof(cnt), hipMemcpyDeviceToHost, st));
    if ((rc = d_hori.finish(st))) return rc;
    if ((rc = d_dist.finish(st))) return rc;
    HZ_HIP(hipStreamSynchronize(st));
    if (stats) {
        stats->num_rays += cnt[0]; stats->guard_events += cnt[1]; stats->num_cells += cnt[4];
        stats->t_h2d_s += h2d_s; stats->t_kernel_s += (double)ms * 1e-3; stats->t_d2h_s += t_d2h.stop();
        stats->t_total_s += t_total.stop();
        stats->elev_num = tb.elev_num; stats->bvh_height = sc->hdr.height; stats->scene_bytes = sc->hdr.total_bytes;
    }
    if (opts && opts->verbose) {
        printf("Number of locations for which horizon is computed: %d \n", num_loc);
        printf("Ray tracing time: %g s\n", (double)ms * 1e-3);
        printf("Number of rays shot: %llu\n", cnt[0]);
    }
    return HZ_OK;
}

// The distance to the horizon of a stored horizon (hz_horidist.hip; DESIGN.md section 4, clause 16).  hori_kind: bit 0 = planes,
// bit 1 = 16-bit codes.  `hori` and `dist` address inner-domain row 0 (or, opts.hori_is_slab, row_begin) in the layout of the
// kind.  Two device arrays are one launch; a host side moves chunk by chunk through a bounded device buffer (opts.chunk_rows
// rows, else about 1 GiB of horizon and distances together), copy in -- kernel -- copy out on the scene's stream.
static int horidist_run(const Scene *sc, const void *hori, int hori_kind, float *dist, const float *vec_norm,
                        const float *vec_north, int offset_0, int offset_1, int dim_in_0, int dim_in_1, int azim_num,
                        float dist_search, float hori_acc, float elev_ang_low_lim, const uint8_t *mask, float ray_org_elev,
                        const hz_opts *opts, hz_stats *stats) {
    int rc = HZ_OK;
    if (hori_kind < 0 || hori_kind > 3) return set_error(HZ_ERR_ARG, "hori_kind must be 0 ... 3 (bit 0: planes, bit 1: 16-bit codes)");
    const bool planes = (hori_kind & HZ_HORI_PLANES) != 0, q16 = (hori_kind & HZ_HORI_U16) != 0;
    const size_t es = q16 ? sizeof(uint16_t) : sizeof(float);
    if (!hori || !dist) return set_error(HZ_ERR_ARG, "hori and dist must not be NULL");
    if ((reinterpret_cast<uintptr_t>(hori) & (es - 1)) || (reinterpret_cast<uintptr_t>(dist) & 3))
        return set_error(HZ_ERR_ARG, "hori or dist is not aligned to its element type");
    if (!vec_norm || !vec_north || !mask) return set_error(HZ_ERR_ARG, "vec_norm, vec_north and mask must not be NULL");
    if (dim_in_0 <= 0 || dim_in_1 <= 0 || azim_num <= 0) return set_error(HZ_ERR_ARG, "dim_in_0, dim_in_1 and azim_num must be positive");
    if (offset_0 < 0 || offset_1 < 0 || offset_0 + dim_in_0 > sc->hdr.d0 || offset_1 + dim_in_1 > sc->hdr.d1)
        return set_error(HZ_ERR_ARG, "inconsistency between input arguments dem_dim_0, dem_dim_1, offset_0, offset_1 and vec_norm");
    if (!(hori_acc > 0.0f) || hori_acc > 10.0f) return set_error(HZ_ERR_ARG, "limit of hori_acc (10 degree) is exceeded");
    int row_begin, row_end;
    if ((rc = resolve_row_slab(opts, dim_in_0, &row_begin, &row_end)) || row_begin == row_end) return rc;
    HZ_HIP(hipSetDevice(sc->device));
    std::lock_guard<std::mutex> run_lock(sc->run_mu);
    hipStream_t st = sc->stream;
    Timer t_total; t_total.start();
    HostTables tb;
    build_tables(azim_num, hori_acc, elev_ang_low_lim, tb);
    if (tb.elev_num < 2) return set_error(HZ_ERR_ARG, "elevation table is empty (elev_ang_low_lim too high)");
    const float dist_m = (float)((double)dist_search * 1000.0);

    const size_t A = (size_t)azim_num;
    const size_t ncell = (size_t)dim_in_0 * dim_in_1, slab_cells = (size_t)(row_end - row_begin) * dim_in_1;
    Timer t_h2d; t_h2d.start();
    DevIn<float> d_norm, d_north;
    DevIn<uint8_t> d_mask;
    DevTables dt;
    const bool inputs_are_slab = opts && opts->inputs_are_slab;
    const size_t in_off = (size_t)row_begin * dim_in_1, src_off = inputs_are_slab ? 0 : in_off;
    if ((rc = d_norm.bind(vec_norm + 3 * src_off, slab_cells * 3, st))) return rc;
    if ((rc = d_north.bind(vec_north + 3 * src_off, slab_cells * 3, st))) return rc;
    if ((rc = d_mask.bind(mask + src_off, slab_cells, st))) return rc;
    if ((rc = dt.bind(tb, false, st))) return rc;
    DevBuf d_cnt;
    HZ_HIP(d_cnt.alloc(2 * sizeof(unsigned long long)));
    HZ_HIP(hipMemsetAsync(d_cnt.p, 0, 2 * sizeof(unsigned long long), st));
    const bool hori_is_slab = opts && opts->hori_is_slab;
    const size_t plane_stride = hori_is_slab ? slab_cells : ncell;
    const size_t cell_base = hori_is_slab ? 0 : in_off;      // the slab's first cell in hori / dist
    const bool h_dev = is_device_ptr(hori), d_dev = is_device_ptr(dist);
    const size_t row_in = (size_t)dim_in_1 * A * es, row_out = (size_t)dim_in_1 * A * sizeof(float);
    int chunk_rows = row_end - row_begin;
    if (!(h_dev && d_dev)) {
        if (opts && opts->chunk_rows > 0) chunk_rows = std::min(chunk_rows, opts->chunk_rows);
        else chunk_rows = (int)std::max<size_t>(1, std::min<size_t>((size_t)chunk_rows, ((size_t)1 << 30) / (row_in + row_out)));
    }
    DevBuf tmp_in, tmp_out;
    size_t tmp_bytes = 0;
    if (!h_dev) { HZ_HIP(tmp_in.alloc((size_t)chunk_rows * row_in)); tmp_bytes += (size_t)chunk_rows * row_in; }
    if (!d_dev) { HZ_HIP(tmp_out.alloc((size_t)chunk_rows * row_out)); tmp_bytes += (size_t)chunk_rows * row_out; }
    HZ_HIP(hipStreamSynchronize(st));
    double h2d_s = t_h2d.stop();

    HoridistArgs a;
    a.vec_norm = d_norm.dev - 3 * in_off; a.vec_north = d_north.dev - 3 * in_off; a.mask = d_mask.dev - in_off;
    a.q16 = q16 ? 1 : 0; a.planes = planes ? 1 : 0;
    a.offset_0 = offset_0; a.offset_1 = offset_1; a.dim_in_1 = dim_in_1;
    a.azim_num = azim_num; a.elev_num = tb.elev_num;
    a.hori_acc = tb.hori_acc; a.up = tb.up; a.dist_m = dist_m; a.ray_org_elev = ray_org_elev;
    a.azim_sin = dt.azim_sin.dev; a.azim_cos = dt.azim_cos.dev; a.elev_ang = dt.elev_ang.dev; a.elev_sin = dt.elev_sin.dev; a.elev_cos = dt.elev_cos.dev;
    a.block_w = g_horidist_block_w.load(std::memory_order_relaxed);
    a.counters = static_cast<unsigned long long *>(d_cnt.p);
    Event ev[4];      // copy in -- kernel -- copy out
    float ms_in = 0.0f, ms_kernel = 0.0f, ms_out = 0.0f;
    const char *hori_b = static_cast<const char *>(hori);
    for (int rb = row_begin; rb < row_end; rb += chunk_rows) {
        const int re = std::min(rb + chunk_rows, row_end);
        const size_t cc = (size_t)(re - rb) * dim_in_1, c0 = cell_base + (size_t)(rb - row_begin) * dim_in_1;
        a.row_begin = rb; a.row_end = re;
        if ((rc = ev[0].record(st))) return rc;
        if (h_dev) {
            a.hori = planes ? hori : static_cast<const void *>(hori_b + c0 * A * es);
            a.hori_stride = plane_stride; a.hori_cell0 = c0;
        } else {
            if (planes) HZ_HIP(hipMemcpy2DAsync(tmp_in.p, cc * es, hori_b + c0 * es, plane_stride * es, cc * es, A, hipMemcpyHostToDevice, st));
            else HZ_HIP(hipMemcpyAsync(tmp_in.p, hori_b + c0 * A * es, cc * A * es, hipMemcpyHostToDevice, st));
            a.hori = tmp_in.p; a.hori_stride = cc; a.hori_cell0 = 0;
        }
        if (d_dev) { a.dist = planes ? dist : dist + c0 * A; a.dist_stride = plane_stride; a.dist_cell0 = c0; }
        else { a.dist = static_cast<float *>(tmp_out.p); a.dist_stride = cc; a.dist_cell0 = 0; }
        if ((rc = ev[1].record(st))) return rc;
        if ((rc = horidist_launch(sc, a, st))) { (void)hipStreamSynchronize(st); return rc; }
        if ((rc = ev[2].record(st))) return rc;
        if (!d_dev) {
            if (planes) HZ_HIP(hipMemcpy2DAsync(dist + c0, plane_stride * sizeof(float), tmp_out.p, cc * sizeof(float), cc * sizeof(float), A,
                                                hipMemcpyDeviceToHost, st));
            else HZ_HIP(hipMemcpyAsync(dist + c0 * A, tmp_out.p, cc * A * sizeof(float), hipMemcpyDeviceToHost, st));
        }
        if ((rc = ev[3].record(st))) return rc;
        if (hipStreamSynchronize(st) != hipSuccess)
            return set_error(HZ_ERR_HIP, "horizon distance kernel failed: %s", hipGetErrorString(hipGetLastError()));
        ms_in += ev[0].ms_until(ev[1]); ms_kernel += ev[1].ms_until(ev[2]); ms_out += ev[2].ms_until(ev[3]);
    }
    unsigned long long cnt[2] = {0, 0};
    HZ_HIP(hipMemcpy(cnt, d_cnt.p, sizeof(cnt), hipMemcpyDeviceToHost));
    if (stats) {
        stats->num_rays += cnt[0]; stats->num_cells += cnt[1];
        stats->t_kernel_s += (double)ms_kernel * 1e-3;
        stats->t_h2d_s += h2d_s + (double)ms_in * 1e-3; stats->t_d2h_s += (double)ms_out * 1e-3;
        stats->t_total_s += t_total.stop();
        stats->elev_num = tb.elev_num; stats->bvh_height = sc->hdr.height; stats->scene_bytes = sc->hdr.total_bytes;
        stats->scratch_bytes = (uint64_t)tmp_bytes;
    }
    return HZ_OK;
}

// A one-shot call: scene, `call(scene, stats of the call)`, release; the scene build is in its hz_stats, t_total_s is the whole call's
template <typename F>
static int one_shot(const float *vert_grid, int dem_dim_0, int dem_dim_1, const char *geom_type, const float *vert_simp,
                    int num_vert_simp, const int32_t *tri_ind_simp, int num_tri_simp, const hz_opts *opts, hz_stats *stats, F call) {
    Timer t; t.start();
    hz_scene *scene = nullptr;
    hz_stats local;
    memset(&local, 0, sizeof(local));
    int rc = hz_scene_create(vert_grid, dem_dim_0, dem_dim_1, geom_type, vert_simp, num_vert_simp,
                             tri_ind_simp, num_tri_simp, opts ? opts->device : 0, &scene, &local);
    if (rc) return rc;
    rc = call(scene, &local);
    hz_scene_destroy(scene);
    local.t_total_s = t.stop();
    if (stats) *stats = local;
    return rc;
}

}  // namespace hz

using namespace hz;

extern "C" {

// The gridded entry points: check what needs no device, describe the call, run it.  Every one of them names its arguments alike:
// the HorizonCall of those arguments with the output (hori, hori_kind, dist)
#define HZ_GRIDDED_CALL(...)                                                                                             \
    HorizonCall{vec_norm, vec_north, offset_0, offset_1, dim_in_0, dim_in_1, azim_num, dist_search, hori_acc, ray_algorithm, \
                elev_ang_low_lim, mask, hori_fill, ray_org_elev, opts, topo, stats, HoriOut{__VA_ARGS__}}

static int scene_call(const hz_scene *scene, const HorizonCall &c) {
    if (!scene) return set_error(HZ_ERR_ARG, "scene is NULL");
    return horizon_run(reinterpret_cast<const Scene *>(scene), c);
}

// the one-shot call: scene, horizon, release
static int gridded_one_shot(const float *vert_grid, int dem_dim_0, int dem_dim_1, const char *geom_type, const float *vert_simp,
                            int num_vert_simp, const int32_t *tri_ind_simp, int num_tri_simp, HorizonCall c) {
    Timer t; t.start();
    const bool verbose = c.opts && c.opts->verbose;
    if (verbose) {   // horizon_comp.cpp:643-645 (the engine named there is Embree)
        printf("--------------------------------------------------------\n");
        printf("Horizon computation with libhorayzon_hip (LBVH on MI355X)\n");
        printf("--------------------------------------------------------\n");
    }
    hz_scene *scene = nullptr;
    hz_stats local, *stats = c.stats;
    memset(&local, 0, sizeof(local));
    int rc = hz_scene_create(vert_grid, dem_dim_0, dem_dim_1, geom_type, vert_simp, num_vert_simp,
                             tri_ind_simp, num_tri_simp, c.opts ? c.opts->device : 0, &scene, &local);
    if (rc) return rc;
    if (verbose) {   // horizon_comp.cpp:113-114, :133-135 / :156-158 / :177, :201-203, :227, :664
        printf("DEM dimensions: (%d, %d) \n", dem_dim_0, dem_dim_1);
        printf("Number of vertices: %d \n", dem_dim_0 * dem_dim_1);
        const int nq = (dem_dim_0 - 1) * (dem_dim_1 - 1);
        if (strcmp(geom_type, "triangle") == 0) { printf("Selected geometry type: triangle\n"); printf("Number of triangles: %d \n", nq * 2); }
        else if (strcmp(geom_type, "quad") == 0) { printf("Selected geometry type: quad\n"); printf("Number of quads: %d \n", nq); }
        else printf("Selected geometry type: grid\n");
        if (num_vert_simp >= 3) {
            printf("Add triangles for outer simplified domain\n");
            printf("- number of verties: %d \n", num_vert_simp);
            printf("- number of triangles: %d \n", num_tri_simp);
        }
        printf("BVH build time: %g s\n", local.t_bvh_s);
        printf("Total initialisation time: %g s\n", t.stop());
    }
    c.stats = &local;
    rc = scene_call(scene, c);
    hz_scene_destroy(scene);   // the reference also releases the scene per call, horizon_comp.cpp:813-814
    local.t_total_s = t.stop();
    if (verbose) {   // :818-820
        printf("Total run time: %g s\n", local.t_total_s);
        printf("--------------------------------------------------------\n");
        fflush(stdout);
    }
    if (stats) *stats = local;
    return rc;
}

int hz_horizon_gridded_scene_ex(const hz_scene *scene, const float *vec_norm, const float *vec_north,
                                int offset_0, int offset_1, float *hori_buffer, int dim_in_0, int dim_in_1,
                                int azim_num, float dist_search, float hori_acc, const char *ray_algorithm,
                                float elev_ang_low_lim, const uint8_t *mask, float hori_fill,
                                float ray_org_elev, const hz_opts *opts, const hz_topo_out *topo, hz_stats *stats) {
    return scene_call(scene, HZ_GRIDDED_CALL(hori_buffer, 0, nullptr));
}

int hz_horizon_gridded_scene(const hz_scene *scene, const float *vec_norm, const float *vec_north,
                             int offset_0, int offset_1, float *hori_buffer, int dim_in_0, int dim_in_1,
                             int azim_num, float dist_search, float hori_acc, const char *ray_algorithm,
                             float elev_ang_low_lim, const uint8_t *mask, float hori_fill,
                             float ray_org_elev, const hz_opts *opts, hz_stats *stats) {
    const hz_topo_out *topo = nullptr;
    return scene_call(scene, HZ_GRIDDED_CALL(hori_buffer, 0, nullptr));
}

int hz_horizon_gridded_ex(const float *vert_grid, int dem_dim_0, int dem_dim_1, const float *vec_norm,
                          const float *vec_north, int offset_0, int offset_1, float *hori_buffer,
                          int dim_in_0, int dim_in_1, int azim_num, float dist_search, float hori_acc,
                          const char *ray_algorithm, const char *geom_type, const float *vert_simp,
                          int num_vert_simp, const int32_t *tri_ind_simp, int num_tri_simp,
                          float elev_ang_low_lim, const uint8_t *mask, float hori_fill, float ray_org_elev,
                          const hz_opts *opts, const hz_topo_out *topo, hz_stats *stats) {
    return gridded_one_shot(vert_grid, dem_dim_0, dem_dim_1, geom_type, vert_simp, num_vert_simp, tri_ind_simp, num_tri_simp,
                            HZ_GRIDDED_CALL(hori_buffer, 0, nullptr));
}

int hz_horizon_gridded(const float *vert_grid, int dem_dim_0, int dem_dim_1, const float *vec_norm,
                       const float *vec_north, int offset_0, int offset_1, float *hori_buffer,
                       int dim_in_0, int dim_in_1, int azim_num, float dist_search, float hori_acc,
                       const char *ray_algorithm, const char *geom_type, const float *vert_simp,
                       int num_vert_simp, const int32_t *tri_ind_simp, int num_tri_simp,
                       float elev_ang_low_lim, const uint8_t *mask, float hori_fill, float ray_org_elev,
                       const hz_opts *opts, hz_stats *stats) {
    const hz_topo_out *topo = nullptr;
    return gridded_one_shot(vert_grid, dem_dim_0, dem_dim_1, geom_type, vert_simp, num_vert_simp, tri_ind_simp, num_tri_simp,
                            HZ_GRIDDED_CALL(hori_buffer, 0, nullptr));
}

// hori_planes f32[azim_num][rows][dim_in_1] in place of hori_buffer: the checks that need no device, before a scene is built
static int check_planes_call(const float *hori_planes, int dim_in_0, int dim_in_1, int azim_num, const hz_opts *opts) {
    if (!hori_planes) return set_error(HZ_ERR_ARG, "hori_planes is NULL");
    if (dim_in_0 <= 0 || dim_in_1 <= 0 || azim_num <= 0) return set_error(HZ_ERR_ARG, "dim_in_0, dim_in_1 and azim_num must be positive");
    if (opts && opts->skip_hori) return set_error(HZ_ERR_ARG, "skip_hori with hori_planes: there is nothing to lay out");
    return HZ_OK;
}

int hz_horizon_gridded_scene_planes(const hz_scene *scene, const float *vec_norm, const float *vec_north,
                                    int offset_0, int offset_1, float *hori_planes, int dim_in_0, int dim_in_1,
                                    int azim_num, float dist_search, float hori_acc, const char *ray_algorithm,
                                    float elev_ang_low_lim, const uint8_t *mask, float hori_fill,
                                    float ray_org_elev, const hz_opts *opts, const hz_topo_out *topo, hz_stats *stats) {
    if (!scene) return set_error(HZ_ERR_ARG, "scene is NULL");
    const int rc = check_planes_call(hori_planes, dim_in_0, dim_in_1, azim_num, opts);
    return rc ? rc : scene_call(scene, HZ_GRIDDED_CALL(hori_planes, HZ_HORI_PLANES, nullptr));
}

int hz_horizon_gridded_planes(const float *vert_grid, int dem_dim_0, int dem_dim_1, const float *vec_norm,
                              const float *vec_north, int offset_0, int offset_1, float *hori_planes,
                              int dim_in_0, int dim_in_1, int azim_num, float dist_search, float hori_acc,
                              const char *ray_algorithm, const char *geom_type, const float *vert_simp,
                              int num_vert_simp, const int32_t *tri_ind_simp, int num_tri_simp,
                              float elev_ang_low_lim, const uint8_t *mask, float hori_fill, float ray_org_elev,
                              const hz_opts *opts, const hz_topo_out *topo, hz_stats *stats) {
    const int rc = check_planes_call(hori_planes, dim_in_0, dim_in_1, azim_num, opts);
    return rc ? rc : gridded_one_shot(vert_grid, dem_dim_0, dem_dim_1, geom_type, vert_simp, num_vert_simp, tri_ind_simp, num_tri_simp,
                                      HZ_GRIDDED_CALL(hori_planes, HZ_HORI_PLANES, nullptr));
}

// hori_q u16[rows][dim_in_1][azim_num] or (planes) u16[azim_num][rows][dim_in_1] in place of hori_buffer: as check_planes_call
static int check_q16_call(const uint16_t *hori_q, int planes, int dim_in_0, int dim_in_1, int azim_num, const hz_opts *opts) {
    if (!hori_q) return set_error(HZ_ERR_ARG, "hori_q is NULL");
    if (reinterpret_cast<uintptr_t>(hori_q) & 1) return set_error(HZ_ERR_ARG, "hori_q is not aligned to 2 bytes");
    if (planes != 0 && planes != 1) return set_error(HZ_ERR_ARG, "planes must be 0 or 1");
    if (dim_in_0 <= 0 || dim_in_1 <= 0 || azim_num <= 0) return set_error(HZ_ERR_ARG, "dim_in_0, dim_in_1 and azim_num must be positive");
    if (opts && opts->skip_hori) return set_error(HZ_ERR_ARG, "skip_hori with hori_q: there is nothing to lay out");
    return HZ_OK;
}

int hz_horizon_gridded_scene_q16(const hz_scene *scene, const float *vec_norm, const float *vec_north,
                                 int offset_0, int offset_1, uint16_t *hori_q, int planes, int dim_in_0, int dim_in_1,
                                 int azim_num, float dist_search, float hori_acc, const char *ray_algorithm,
                                 float elev_ang_low_lim, const uint8_t *mask, float hori_fill,
                                 float ray_org_elev, const hz_opts *opts, const hz_topo_out *topo, hz_stats *stats) {
    if (!scene) return set_error(HZ_ERR_ARG, "scene is NULL");
    const int rc = check_q16_call(hori_q, planes, dim_in_0, dim_in_1, azim_num, opts);
    return rc ? rc : scene_call(scene, HZ_GRIDDED_CALL(hori_q, HZ_HORI_U16 | (planes ? HZ_HORI_PLANES : 0), nullptr));
}

int hz_horizon_gridded_q16(const float *vert_grid, int dem_dim_0, int dem_dim_1, const float *vec_norm,
                           const float *vec_north, int offset_0, int offset_1, uint16_t *hori_q, int planes,
                           int dim_in_0, int dim_in_1, int azim_num, float dist_search, float hori_acc,
                           const char *ray_algorithm, const char *geom_type, const float *vert_simp,
                           int num_vert_simp, const int32_t *tri_ind_simp, int num_tri_simp,
                           float elev_ang_low_lim, const uint8_t *mask, float hori_fill, float ray_org_elev,
                           const hz_opts *opts, const hz_topo_out *topo, hz_stats *stats) {
    const int rc = check_q16_call(hori_q, planes, dim_in_0, dim_in_1, azim_num, opts);
    return rc ? rc : gridded_one_shot(vert_grid, dem_dim_0, dem_dim_1, geom_type, vert_simp, num_vert_simp, tri_ind_simp, num_tri_simp,
                                      HZ_GRIDDED_CALL(hori_q, HZ_HORI_U16 | (planes ? HZ_HORI_PLANES : 0), nullptr));
}

// `hori` of hori_kind (bit 0: planes, bit 1: 16-bit codes) plus the distances: the checks that need no device
static int check_dist_call(const void *hori, int hori_kind, const float *dist_buffer, int dim_in_0, int dim_in_1, int azim_num,
                           const hz_opts *opts) {
    if (hori_kind < 0 || hori_kind > 3) return set_error(HZ_ERR_ARG, "hori_kind must be 0 ... 3 (bit 0: planes, bit 1: 16-bit codes)");
    if (!hori) return set_error(HZ_ERR_ARG, "hori is NULL");
    if (!dist_buffer) return set_error(HZ_ERR_ARG, "dist_buffer is NULL");
    if ((hori_kind & HZ_HORI_U16) && (reinterpret_cast<uintptr_t>(hori) & 1)) return set_error(HZ_ERR_ARG, "hori is not aligned to 2 bytes");
    if (dim_in_0 <= 0 || dim_in_1 <= 0 || azim_num <= 0) return set_error(HZ_ERR_ARG, "dim_in_0, dim_in_1 and azim_num must be positive");
    if (opts && opts->skip_hori) return set_error(HZ_ERR_ARG, "skip_hori with dist_buffer: there is no horizon to return it with");
    return HZ_OK;
}

int hz_horizon_gridded_scene_dist(const hz_scene *scene, const float *vec_norm, const float *vec_north,
                                  int offset_0, int offset_1, void *hori, int hori_kind, float *dist_buffer,
                                  int dim_in_0, int dim_in_1, int azim_num, float dist_search, float hori_acc,
                                  const char *ray_algorithm, float elev_ang_low_lim, const uint8_t *mask, float hori_fill,
                                  float ray_org_elev, const hz_opts *opts, const hz_topo_out *topo, hz_stats *stats) {
    if (!scene) return set_error(HZ_ERR_ARG, "scene is NULL");
    const int rc = check_dist_call(hori, hori_kind, dist_buffer, dim_in_0, dim_in_1, azim_num, opts);
    return rc ? rc : scene_call(scene, HZ_GRIDDED_CALL(hori, hori_kind, dist_buffer));
}

int hz_horizon_gridded_dist(const float *vert_grid, int dem_dim_0, int dem_dim_1, const float *vec_norm,
                            const float *vec_north, int offset_0, int offset_1, void *hori, int hori_kind,
                            float *dist_buffer, int dim_in_0, int dim_in_1, int azim_num, float dist_search, float hori_acc,
                            const char *ray_algorithm, const char *geom_type, const float *vert_simp,
                            int num_vert_simp, const int32_t *tri_ind_simp, int num_tri_simp,
                            float elev_ang_low_lim, const uint8_t *mask, float hori_fill, float ray_org_elev,
                            const hz_opts *opts, const hz_topo_out *topo, hz_stats *stats) {
    const int rc = check_dist_call(hori, hori_kind, dist_buffer, dim_in_0, dim_in_1, azim_num, opts);
    return rc ? rc : gridded_one_shot(vert_grid, dem_dim_0, dem_dim_1, geom_type, vert_simp, num_vert_simp, tri_ind_simp, num_tri_simp,
                                      HZ_GRIDDED_CALL(hori, hori_kind, dist_buffer));
}
#undef HZ_GRIDDED_CALL

int hz_horizon_distance_scene(const hz_scene *scene, const void *hori, int hori_kind, float *dist,
                              const float *vec_norm, const float *vec_north, int offset_0, int offset_1,
                              int dim_in_0, int dim_in_1, int azim_num, float dist_search, float hori_acc,
                              float elev_ang_low_lim, const uint8_t *mask, float ray_org_elev,
                              const hz_opts *opts, hz_stats *stats) {
    if (!scene) return set_error(HZ_ERR_ARG, "scene is NULL");
    return horidist_run(reinterpret_cast<const Scene *>(scene), hori, hori_kind, dist, vec_norm, vec_north, offset_0, offset_1,
                        dim_in_0, dim_in_1, azim_num, dist_search, hori_acc, elev_ang_low_lim, mask, ray_org_elev, opts, stats);
}

int hz_horizon_distance(const float *vert_grid, int dem_dim_0, int dem_dim_1, const void *hori, int hori_kind, float *dist,
                        const float *vec_norm, const float *vec_north, int offset_0, int offset_1,
                        int dim_in_0, int dim_in_1, int azim_num, float dist_search, float hori_acc,
                        const char *geom_type, const float *vert_simp, int num_vert_simp,
                        const int32_t *tri_ind_simp, int num_tri_simp, float elev_ang_low_lim, const uint8_t *mask,
                        float ray_org_elev, const hz_opts *opts, hz_stats *stats) {
    if (!hori || !dist) return set_error(HZ_ERR_ARG, "hori and dist must not be NULL");
    return one_shot(vert_grid, dem_dim_0, dem_dim_1, geom_type, vert_simp, num_vert_simp, tri_ind_simp, num_tri_simp, opts, stats,
                    [&](const hz_scene *scene, hz_stats *st) {
        return hz_horizon_distance_scene(scene, hori, hori_kind, dist, vec_norm, vec_north, offset_0, offset_1, dim_in_0, dim_in_1,
                                         azim_num, dist_search, hori_acc, elev_ang_low_lim, mask, ray_org_elev, opts, st);
    });
}

int hz_horizon_locations_scene(const hz_scene *scene, const float *coords, const float *vec_norm,
                               const float *vec_north, float *hori_buffer, float *hori_dist_buffer, int num_loc,
                               int azim_num, float dist_search, float hori_acc, const char *ray_algorithm,
                               float elev_ang_low_lim, const float *ray_org_elev, int hori_dist_out,
                               const hz_opts *opts, hz_stats *stats) {
    if (!scene) return set_error(HZ_ERR_ARG, "scene is NULL");
    return locations_run(reinterpret_cast<const Scene *>(scene), coords, vec_norm, vec_north, hori_buffer,
                         hori_dist_buffer, num_loc, azim_num, dist_search, hori_acc, ray_algorithm,
                         elev_ang_low_lim, ray_org_elev, hori_dist_out, opts, stats);
}

int hz_horizon_locations(const float *vert_grid, int dem_dim_0, int dem_dim_1, const float *coords,
                         const float *vec_norm, const float *vec_north, float *hori_buffer,
                         float *hori_dist_buffer, int num_loc, int azim_num, float dist_search, float hori_acc,
                         const char *ray_algorithm, const char *geom_type, float elev_ang_low_lim,
                         const float *ray_org_elev, int hori_dist_out, const hz_opts *opts, hz_stats *stats) {
    // no simplified outer mesh for locations: horizon_comp.cpp:848-852
    return one_shot(vert_grid, dem_dim_0, dem_dim_1, geom_type, nullptr, 0, nullptr, 0, opts, stats,
                    [&](const hz_scene *scene, hz_stats *st) {
        return hz_horizon_locations_scene(scene, coords, vec_norm, vec_north, hori_buffer, hori_dist_buffer, num_loc, azim_num,
                                          dist_search, hori_acc, ray_algorithm, elev_ang_low_lim, ray_org_elev, hori_dist_out, opts, st);
    });
}

int hz_horizon_tables(int azim_num, float hori_acc, float elev_ang_low_lim, float *azim_sin,
                      float *azim_cos, int elev_cap, float *elev_ang, float *elev_sin, float *elev_cos,
                      int *elev_num) {
    if (azim_num <= 0 || !(hori_acc > 0.0f)) return set_error(HZ_ERR_ARG, "azim_num and hori_acc must be positive");
    HostTables t;
    build_tables(azim_num, hori_acc, elev_ang_low_lim, t);
    if (elev_num) *elev_num = t.elev_num;
    if (azim_sin) memcpy(azim_sin, t.azim_sin.data(), sizeof(float) * (size_t)azim_num);
    if (azim_cos) memcpy(azim_cos, t.azim_cos.data(), sizeof(float) * (size_t)azim_num);
    if (elev_ang && elev_sin && elev_cos && t.elev_num > 0 && t.elev_num <= elev_cap) {
        memcpy(elev_ang, t.elev_ang.data(), sizeof(float) * (size_t)t.elev_num);
        memcpy(elev_sin, t.elev_sin.data(), sizeof(float) * (size_t)t.elev_num);
        memcpy(elev_cos, t.elev_cos.data(), sizeof(float) * (size_t)t.elev_num);
    }
    return HZ_OK;
}

}  // extern "C"
