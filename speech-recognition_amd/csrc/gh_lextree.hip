// Lexical-tree spell check: the string-edit Viterbi over a flattened prefix tree (reference: text_viterbi,
// sr/langmodel/spellchecker.py).  Every cost is a small non-negative integer, so the kernels compute in integers and
// the results equal the reference's float64 ones exactly.
//
// Rows.  The host flattens the tree in preorder: row 0 the root, 1..R-2 the tree, R-1 the extra space row.  At creation
// the rows are renumbered by DEPTH LEVEL: new row 0 = root, 1 = space, then level 1, level 2, ... each level starting
// on a multiple of 64 and padded to one (pad rows have parent -1).  A wave then always owns 64 rows of one level.
//
// Recurrence (column c of x' = '*' + x, d = dist(x'[c], val[r]), ties to the first option listed):
//   root   c > 0: d + 1 + min_k cost[word_end[k], c-1]      (k over all word ends, the space row k = 0 included)
//   space  c > 0: d + min_{k >= 1} cost[word_end[k], c-1]   (c = 0: no value, unless the root itself is a word end)
//   other rows: deletion d + 1 + cost[r, c-1] (c > 0), match d + cost[parent, c-1] (c > 0, parent not the root),
//               insertion d + 1 + cost[parent, c].
// One workgroup per string.  Per column: (A) stage the distance row of x'[c] in LDS and reduce the previous column over
// the word ends ((cost, rank) pairs: the first argmin wins), (B) every thread derives root and space from the partials,
// (C) the levels in order, one barrier each: min(deletion, match) and then the insertion from the parent, whose level
// is complete.  The two cost columns live in LDS as uint16 when the host's bound (Dmax+1)(depth+C+1) fits 16 bits and
// the columns fit the CU's 160 KB, else as uint32 in global memory.  Decisions: two ballots per 64-row chunk (low and
// high bit of 0 deletion / 1 match / 2 insertion), plus (root argmin, space argmin) per column.  A second kernel walks
// them back, one lane per string, and returns the rows whose values the host joins.
#include "gh_internal.h"
#include "gh_host.h"
#include <stdlib.h>
#include <string.h>

struct gh_lextree {
    gh_ctx* ctx;
    int R;              // preorder rows, space row included
    int Rp;             // rows of the level numbering (padded)
    int n_levels;       // depth of the tree (levels 1..n_levels)
    int n_we;           // word ends, the space row first
    int n_val;          // distinct node values
    int root_end;       // the root itself is a word end (property 2)
    int max_width;      // widest level (padded)
    int root_code, space_code;   // value codes of the root and the space row
    void* d_arena;
    int2* d_meta;       // [Rp] {parent (level numbering; -1: root, space, pad), value code}
    int32_t* d_we;      // [n_we] word ends (level numbering)
    int32_t* d_pre;     // [Rp] level numbering -> preorder row (-1: pad)
    int32_t* d_lvl;     // [n_levels + 2] first row of every level, then Rp
};

namespace {

constexpr int LT_THREADS = 1024;
constexpr int LT_MAX_VAL = 16384;      // distinct values: the distance row is staged in LDS
constexpr size_t LT_LDS_MAX = 160 * 1024;

struct lt_fwd_args {
    const int2* meta;
    const int32_t* we;
    const int32_t* lvl;
    int Rp, n_levels, n_we, n_val, root_end, code_root, code_space;
    const int64_t* offsets;    // [chunk strings + 1] into codes (x' = '*' + x)
    int64_t code_base;         // offsets[0] of the chunk: column arguments are indexed from it
    const int32_t* codes;
    const uint32_t* dist;      // [n_x, n_val]
    const int64_t* dec_off;    // [chunk strings] first decision pair of each string
    uint64_t* dec;             // [sum C * nchunk][2]
    int2* colarg;              // [sum C] (root argmin, space argmin) of the chunk's columns
    void* gstate;              // uint32 form: [chunk strings][2][Rp]
    int64_t* best_cost;        // [chunk strings]
    int32_t* start;            // [chunk strings] the word end the back-trace starts from (level numbering)
};

struct lt_back_args {
    const int2* meta;
    const int32_t* we;
    const int32_t* pre;
    int nchunk, n;
    const int64_t* offsets;
    const int64_t* dec_off;
    const uint64_t* dec;
    int64_t code_base;
    const int2* colarg;
    const int32_t* start;
    const int64_t* path_off;   // [chunk strings + 1]
    int32_t* path;
    int32_t* path_len;
};

__device__ __forceinline__ uint64_t lt_wave_min(uint64_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t lo = __shfl_xor((unsigned)(v & 0xffffffffu), o, 64);
        const uint32_t hi = __shfl_xor((unsigned)(v >> 32), o, 64);
        const uint64_t w = ((uint64_t)hi << 32) | lo;
        v = w < v ? w : v;
    }
    return v;
}

// min over word ends k in [k0, n_we) of (cost[we[k]] << 32 | k), for the whole workgroup: every thread gets the result
template <typename T>
__device__ __forceinline__ uint64_t lt_we_argmin(const T* col, const int32_t* we, int k0, int n_we, uint64_t* red) {
    const int tid = threadIdx.x, nw = blockDim.x >> 6;
    uint64_t m = ~0ull;
    for (int k = k0 + tid; k < n_we; k += blockDim.x) {
        const uint64_t key = ((uint64_t)(uint32_t)col[we[k]] << 32) | (uint32_t)k;
        m = key < m ? key : m;
    }
    m = lt_wave_min(m);
    if ((tid & 63) == 0) red[tid >> 6] = m;
    __syncthreads();
    uint64_t r = red[0];
    for (int w = 1; w < nw; ++w) r = red[w] < r ? red[w] : r;
    return r;
}

template <typename T, bool IN_LDS>
__global__ __launch_bounds__(LT_THREADS) void lextree_fwd_kernel(lt_fwd_args a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lt_lds[];
    const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63;
    const int s = blockIdx.x;
    const int64_t x0 = a.offsets[s];
    const int C = (int)(a.offsets[s + 1] - x0);
    const int Rp = a.Rp, nchunk = Rp >> 6;
    uint64_t* red = reinterpret_cast<uint64_t*>(lt_lds);                       // [16]
    int32_t* lvl = reinterpret_cast<int32_t*>(lt_lds + 128);                  // [n_levels + 2]
    const int lvl_bytes = ((a.n_levels + 2) * 4 + 15) & ~15;
    uint32_t* drow = reinterpret_cast<uint32_t*>(lt_lds + 128 + lvl_bytes);   // [n_val]
    const int drow_bytes = (a.n_val * 4 + 15) & ~15;
    T* st = IN_LDS ? reinterpret_cast<T*>(lt_lds + 128 + lvl_bytes + drow_bytes)
                   : reinterpret_cast<T*>(a.gstate) + (size_t)s * 2 * Rp;
    T* prev = st;
    T* cur = st + Rp;
    const uint32_t INF = (uint32_t)(T)~(T)0;
    uint64_t* dec = a.dec + 2 * a.dec_off[s];
    int2* colarg = a.colarg + (x0 - a.code_base);
    for (int i = tid; i < a.n_levels + 2; i += nt) lvl[i] = a.lvl[i];

    for (int c = 0; c < C; ++c) {
        // (A) distance row of x'[c]; word-end reduction of column c-1 (k >= 1: the space row's candidates)
        const int xc = a.codes[x0 + c];
        for (int v = tid; v < a.n_val; v += nt) drow[v] = a.dist[(size_t)xc * a.n_val + v];
        uint64_t m = ~0ull;
        if (c > 0) m = lt_we_argmin(prev, a.we, 1, a.n_we, red);
        else __syncthreads();
        // (B) root and space
        uint32_t root, space;
        if (c == 0) {
            root = 0;
            space = a.root_end ? drow[a.code_space] : INF;
        } else {
            const uint32_t vmin = (uint32_t)(m >> 32), kmin = (uint32_t)m;
            const uint32_t vsp = prev[1];                         // word end k = 0: the space row
            const bool k0 = vsp <= vmin;
            root = drow[a.code_root] + 1 + (k0 ? vsp : vmin);
            space = drow[a.code_space] + vmin;
            if (tid == 0) colarg[c] = make_int2(k0 ? 0 : (int)kmin, (int)kmin);
        }
        if (tid == 0) { cur[0] = (T)root; cur[1] = (T)space; }
        // (C) the levels: the parent's level is complete (barrier) when a level starts
        for (int L = 1; L <= a.n_levels; ++L) {
            const int lo = lvl[L], hi = lvl[L + 1];
            for (int base = lo + (tid & ~63); base < hi; base += nt) {       // (wave-uniform)
                const int r = base + lane;
                const int2 mt = a.meta[r];
                uint32_t d2 = 0;
                if (mt.x >= 0) {
                    const uint32_t d = drow[mt.y];
                    uint32_t best = 0xffffffffu;
                    if (c > 0) {
                        best = d + 1 + (uint32_t)prev[r];
                        if (mt.x != 0) {
                            const uint32_t mm = d + (uint32_t)prev[mt.x];
                            if (mm < best) { best = mm; d2 = 1; }
                        }
                    }
                    const uint32_t ins = d + 1 + (mt.x == 0 ? root : (uint32_t)cur[mt.x]);
                    if (ins < best) { best = ins; d2 = 2; }
                    cur[r] = (T)best;
                }
                const uint64_t b0 = __ballot(d2 & 1), b1 = __ballot(d2 >> 1);
                if (lane == 0) {
                    uint64_t* w = dec + 2 * ((size_t)c * nchunk + (base >> 6));
                    w[0] = b0;
                    w[1] = b1;
                }
            }
            __syncthreads();
        }
        if (a.n_levels == 0) __syncthreads();
        T* t = prev; prev = cur; cur = t;
    }
    // the end of the decode: first argmin over every word end of the last column
    const uint64_t m = lt_we_argmin(prev, a.we, 0, a.n_we, red);
    if (tid == 0) {
        a.best_cost[s] = (int64_t)(m >> 32);
        a.start[s] = a.we[(uint32_t)m];
    }
}

// one lane per string: (r, C-1) back to column 1 (spellchecker.py's walk); the rows whose value is appended
__global__ __launch_bounds__(64) void lextree_back_kernel(lt_back_args a) {
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= a.n) return;
    const int64_t x0 = a.offsets[s];
    const int C = (int)(a.offsets[s + 1] - x0);
    const uint64_t* dec = a.dec + 2 * a.dec_off[s];
    const int2* colarg = a.colarg + (x0 - a.code_base);
    int32_t* out = a.path + a.path_off[s];
    const int64_t cap = a.path_off[s + 1] - a.path_off[s];
    int r = a.start[s], c = C - 1;
    int64_t n = 0;
    out[n++] = a.pre[r];
    while (c != 1) {
        if (r == 0) {
            r = a.we[colarg[c].x];
            --c;
        } else if (r == 1) {
            r = a.we[colarg[c].y];
            --c;
        } else {
            const uint64_t* w = dec + 2 * ((size_t)c * a.nchunk + (r >> 6));
            const int bit = r & 63;
            const int d = (int)((w[0] >> bit) & 1) | ((int)((w[1] >> bit) & 1) << 1);
            if (d != 0) r = a.meta[r].x;
            if (d != 2) --c;
        }
        if (r != 0) {
            if (n >= cap) { n = -1; break; }   // (cannot happen: the host's bound; kept so that no write goes astray)
            out[n++] = a.pre[r];
        }
    }
    a.path_len[s] = (int32_t)n;
}

size_t lt_lds_bytes(const gh_lextree* t, bool in_lds, int elem) {
    size_t b = 128 + (((size_t)(t->n_levels + 2) * 4 + 15) & ~(size_t)15) + (((size_t)t->n_val * 4 + 15) & ~(size_t)15);
    if (in_lds) b += (size_t)2 * t->Rp * elem;
    return b;
}

}  // namespace

extern "C" int gh_lextree_create(gh_ctx* ctx, int R, const int32_t* parent, const int32_t* val_code, int n_val, int n_word_ends,
                                 const int32_t* word_ends, gh_lextree** out) {
    GH_REQUIRE(ctx && out && parent && val_code && word_ends, "gh_lextree_create: NULL argument");
    *out = nullptr;
    GH_REQUIRE(R >= 2 && R < (1 << 24), "gh_lextree_create: R = %d rows (root .. space row) out of range", R);
    GH_REQUIRE(n_val >= 1 && n_val <= LT_MAX_VAL, "gh_lextree_create: %d distinct values (1..%d)", n_val, LT_MAX_VAL);
    GH_REQUIRE(parent[0] == -1 && parent[R - 1] == -1, "gh_lextree_create: the root and the space row have no parent");
    std::vector<int> depth(R, 0);
    int n_levels = 0;
    for (int r = 1; r < R - 1; ++r) {
        GH_REQUIRE(parent[r] >= 0 && parent[r] < R - 1, "gh_lextree_create: parent[%d] = %d out of range", r, parent[r]);
        // (preorder: a parent precedes its child; a parent at or after its child is a cycle or not a preorder flattening)
        GH_REQUIRE(parent[r] < r, "gh_lextree_create: parent[%d] = %d does not precede its child (cycle)", r, parent[r]);
        depth[r] = depth[parent[r]] + 1;
        n_levels = std::max(n_levels, depth[r]);
    }
    for (int r = 0; r < R; ++r)
        GH_REQUIRE(val_code[r] >= 0 && val_code[r] < n_val, "gh_lextree_create: val_code[%d] = %d out of range", r, val_code[r]);
    GH_REQUIRE(n_word_ends >= 2 && word_ends[0] == R - 1, "gh_lextree_create: word ends must be the space row, then >= 1 tree row");
    for (int k = 1; k < n_word_ends; ++k)
        GH_REQUIRE(word_ends[k] >= 0 && word_ends[k] < R - 1 && (k == 1 || word_ends[k] > word_ends[k - 1]),
                   "gh_lextree_create: bad word end [%d] = %d (tree rows, ascending)", k, word_ends[k]);

    // level numbering: root 0, space 1, level L from lvl[L] (multiples of 64), preorder inside a level
    std::vector<int> width(n_levels + 1, 0);
    for (int r = 1; r < R - 1; ++r) ++width[depth[r]];
    std::vector<int32_t> lvl(n_levels + 2, 0);
    lvl[1] = 64;
    int max_width = 64;
    for (int L = 1; L <= n_levels; ++L) {
        const int w = (width[L] + 63) & ~63;
        lvl[L + 1] = lvl[L] + w;
        max_width = std::max(max_width, w);
    }
    const int Rp = n_levels ? lvl[n_levels + 1] : 64;
    GH_REQUIRE(Rp < (1 << 24), "gh_lextree_create: tree too large");
    std::vector<int32_t> nw(R), fill(lvl.begin(), lvl.end());
    nw[0] = 0;
    nw[R - 1] = 1;
    for (int r = 1; r < R - 1; ++r) nw[r] = fill[depth[r]]++;
    std::vector<int2> meta(Rp, make_int2(-1, 0));
    std::vector<int32_t> pre(Rp, -1), we(n_word_ends);
    for (int r = 0; r < R; ++r) {
        meta[nw[r]] = make_int2((r == 0 || r == R - 1) ? -1 : nw[parent[r]], val_code[r]);
        pre[nw[r]] = r;
    }
    for (int k = 0; k < n_word_ends; ++k) we[k] = nw[word_ends[k]];

    gh_lextree* t = new gh_lextree();
    t->ctx = ctx;
    t->R = R;
    t->Rp = Rp;
    t->n_levels = n_levels;
    t->n_we = n_word_ends;
    t->n_val = n_val;
    t->root_end = word_ends[1] == 0;
    t->max_width = max_width;
    t->root_code = val_code[0];
    t->space_code = val_code[R - 1];
    UploadArena up;
    up.add(&t->d_meta, meta);
    up.add(&t->d_we, we);
    up.add(&t->d_pre, pre);
    up.add(&t->d_lvl, lvl);
    const int rc = up.commit(&t->d_arena);
    if (rc) { delete t; return rc; }
    *out = t;
    return GH_OK;
}

extern "C" void gh_lextree_destroy(gh_lextree* t) {
    if (!t) return;
    if (t->d_arena) (void)hipFree(t->d_arena);
    delete t;
}

extern "C" int gh_text_viterbi(gh_ctx* ctx, const gh_lextree* t, int64_t n_strings, const int64_t* offsets, const int32_t* codes,
                               int n_x_codes, const int64_t* dist_table, int64_t* best_cost, int32_t* path_len,
                               int32_t* path_rows, int64_t path_cap) {
    GH_REQUIRE(ctx && t && t->ctx == ctx, "gh_text_viterbi: NULL context / tree, or a tree of another context");
    GH_REQUIRE(n_strings >= 0, "gh_text_viterbi: n_strings < 0");
    if (n_strings == 0) { ctx->last_chunks = 0; return GH_OK; }
    GH_REQUIRE(offsets && codes && dist_table && best_cost && path_len && path_rows, "gh_text_viterbi: NULL argument");
    GH_REQUIRE(offsets[0] == 0, "gh_text_viterbi: offsets[0] != 0");
    GH_REQUIRE(n_x_codes >= 1 && (int64_t)n_x_codes * t->n_val <= ((int64_t)1 << 28), "gh_text_viterbi: n_x_codes = %d", n_x_codes);
    int64_t Cmax = 0;
    for (int64_t s = 0; s < n_strings; ++s) {
        const int64_t C = offsets[s + 1] - offsets[s];
        GH_REQUIRE(C >= 2 && C < ((int64_t)1 << 30), "gh_text_viterbi: string %lld has %lld columns ('*' + at least one)",
                   (long long)s, (long long)C);
        Cmax = std::max(Cmax, C);
    }
    const int64_t n_codes = offsets[n_strings];
    for (int64_t i = 0; i < n_codes; ++i)
        GH_REQUIRE(codes[i] >= 0 && codes[i] < n_x_codes, "gh_text_viterbi: codes[%lld] = %d out of range", (long long)i, codes[i]);
    const int64_t n_tab = (int64_t)n_x_codes * t->n_val;
    int64_t dmax = 0;
    for (int64_t i = 0; i < n_tab; ++i) {
        GH_REQUIRE(dist_table[i] >= 0, "gh_text_viterbi: dist_table[%lld] = %lld < 0", (long long)i, (long long)dist_table[i]);
        dmax = std::max(dmax, dist_table[i]);
    }
    // every cell <= (Dmax + 1) (depth + C + 1): the cost type is picked so that nothing saturates (all-ones = no value)
    const double bound = ((double)dmax + 1) * ((double)t->n_levels + (double)Cmax + 1);
    if (bound >= 4294967295.0) {
        gh_set_error("gh_text_viterbi: costs up to %.0f do not fit 32 bits", bound);
        return GH_ERR_UNSUPPORTED;
    }
    const char* form_env = getenv("GMMHMM_LEXTREE_FORM");
    const bool force32 = form_env && strcmp(form_env, "32") == 0;
    const bool lds16 = !force32 && bound < 65535.0 && lt_lds_bytes(t, true, 2) <= LT_LDS_MAX;
    const size_t lds = lt_lds_bytes(t, lds16, 2);
    GH_REQUIRE(lds <= LT_LDS_MAX, "gh_text_viterbi: %d distinct values do not fit LDS", t->n_val);
    std::vector<uint32_t> dist(n_tab);
    for (int64_t i = 0; i < n_tab; ++i) dist[i] = (uint32_t)dist_table[i];

    // per string: decision pairs, column arguments, path capacity, (32-bit form) two cost columns
    const int nchunk = t->Rp >> 6;
    std::vector<int64_t> cap(n_strings);     // (a column step plus at most depth insertions per column)
    for (int64_t s = 0; s < n_strings; ++s) cap[s] = 1 + (offsets[s + 1] - offsets[s] - 2) * (int64_t)(t->n_levels + 1);
    auto need = [&](int64_t s) {
        const int64_t C = offsets[s + 1] - offsets[s];
        return (size_t)C * nchunk * 16 + (size_t)C * 12 + (size_t)cap[s] * 4 + 64 + (lds16 ? 0 : (size_t)2 * t->Rp * 4);
    };
    const size_t budget = gh_scratch_budget(ctx);
    std::vector<int64_t> chunk_begin{0};
    size_t acc = 0, biggest = 0;
    for (int64_t s = 0; s < n_strings; ++s) {
        const size_t b = need(s);
        if (s > chunk_begin.back() && acc + b > budget) {
            biggest = std::max(biggest, acc);
            chunk_begin.push_back(s);
            acc = 0;
        }
        acc += b;
    }
    biggest = std::max(biggest, acc);
    chunk_begin.push_back(n_strings);

    // inputs (whole call) + the largest chunk's pieces in one scratch region
    int64_t max_n = 0, max_codes = 0, max_cap = 0;
    for (size_t i = 0; i + 1 < chunk_begin.size(); ++i) {
        const int64_t b = chunk_begin[i], e = chunk_begin[i + 1];
        max_n = std::max(max_n, e - b);
        max_codes = std::max(max_codes, offsets[e] - offsets[b]);
        int64_t cp = 0;
        for (int64_t s = b; s < e; ++s) cp += cap[s];
        max_cap = std::max(max_cap, cp);
    }
    int32_t* d_codes; uint32_t* d_dist; int64_t *d_off, *d_dec_off, *d_path_off, *d_best;
    uint64_t* d_dec; int2* d_colarg; void* d_gstate; int32_t *d_start, *d_path, *d_plen;
    Carver cv;
    cv.add(&d_codes, (size_t)n_codes);
    cv.add(&d_dist, (size_t)n_tab);
    cv.add(&d_off, (size_t)max_n + 1);
    cv.add(&d_dec_off, (size_t)max_n);
    cv.add(&d_path_off, (size_t)max_n + 1);
    cv.add(&d_best, (size_t)max_n);
    cv.add(&d_start, (size_t)max_n);
    cv.add(&d_plen, (size_t)max_n);
    cv.add(&d_colarg, (size_t)max_codes);
    cv.add(&d_path, (size_t)max_cap);
    int64_t max_dec = 0;
    for (size_t i = 0; i + 1 < chunk_begin.size(); ++i)
        max_dec = std::max(max_dec, (offsets[chunk_begin[i + 1]] - offsets[chunk_begin[i]]) * (int64_t)nchunk);
    cv.add(&d_dec, (size_t)max_dec * 2);
    cv.add(reinterpret_cast<uint32_t**>(&d_gstate), lds16 ? 1 : (size_t)max_n * 2 * t->Rp);
    int rc = cv.commit(ctx);
    if (rc) return rc;
    GH_HIP(hipMemcpyAsync(d_codes, codes, (size_t)n_codes * 4, hipMemcpyHostToDevice, ctx->stream));
    GH_HIP(hipMemcpyAsync(d_dist, dist.data(), (size_t)n_tab * 4, hipMemcpyHostToDevice, ctx->stream));

    const int threads = std::min(LT_THREADS, std::max(t->max_width, 64));
    std::vector<int64_t> h_off, h_dec_off, h_path_off;
    std::vector<int32_t> h_path;
    int64_t written = 0;
    for (size_t ci = 0; ci + 1 < chunk_begin.size(); ++ci) {
        const int64_t b = chunk_begin[ci], e = chunk_begin[ci + 1], n = e - b;
        h_off.assign(n + 1, 0);
        h_dec_off.assign(n, 0);
        h_path_off.assign(n + 1, 0);
        for (int64_t s = 0; s < n; ++s) {
            const int64_t C = offsets[b + s + 1] - offsets[b + s];
            h_off[s + 1] = h_off[s] + C;
            h_dec_off[s] = h_off[s] * nchunk;
            h_path_off[s + 1] = h_path_off[s] + cap[b + s];
        }
        for (int64_t s = 0; s <= n; ++s) h_off[s] += offsets[b];   // (into the whole call's codes)
        GH_HIP(hipMemcpyAsync(d_off, h_off.data(), (size_t)(n + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
        GH_HIP(hipMemcpyAsync(d_dec_off, h_dec_off.data(), (size_t)n * 8, hipMemcpyHostToDevice, ctx->stream));
        GH_HIP(hipMemcpyAsync(d_path_off, h_path_off.data(), (size_t)(n + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
        lt_fwd_args fa;
        fa.meta = t->d_meta; fa.we = t->d_we; fa.lvl = t->d_lvl;
        fa.Rp = t->Rp; fa.n_levels = t->n_levels; fa.n_we = t->n_we; fa.n_val = t->n_val; fa.root_end = t->root_end;
        fa.offsets = d_off; fa.codes = d_codes; fa.dist = d_dist; fa.dec_off = d_dec_off; fa.dec = d_dec;
        fa.code_base = offsets[b]; fa.colarg = d_colarg;
        fa.gstate = d_gstate; fa.best_cost = d_best; fa.start = d_start;
        fa.code_root = t->root_code;
        fa.code_space = t->space_code;
        if (lds16) hipLaunchKernelGGL((lextree_fwd_kernel<uint16_t, true>), dim3((unsigned)n), dim3(threads), lds, ctx->stream, fa);
        else hipLaunchKernelGGL((lextree_fwd_kernel<uint32_t, false>), dim3((unsigned)n), dim3(threads), lds, ctx->stream, fa);
        GH_HIP(hipGetLastError());
        lt_back_args ba;
        ba.meta = t->d_meta; ba.we = t->d_we; ba.pre = t->d_pre; ba.nchunk = nchunk; ba.n = (int)n;
        ba.offsets = d_off; ba.dec_off = d_dec_off; ba.dec = d_dec; ba.code_base = offsets[b]; ba.colarg = d_colarg; ba.start = d_start;
        ba.path_off = d_path_off; ba.path = d_path; ba.path_len = d_plen;
        hipLaunchKernelGGL(lextree_back_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, ctx->stream, ba);
        GH_HIP(hipGetLastError());
        h_path.resize(h_path_off[n]);
        GH_HIP(hipMemcpyAsync(best_cost + b, d_best, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream));
        GH_HIP(hipMemcpyAsync(path_len + b, d_plen, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
        GH_HIP(hipMemcpyAsync(h_path.data(), d_path, (size_t)h_path_off[n] * 4, hipMemcpyDeviceToHost, ctx->stream));
        GH_HIP(hipStreamSynchronize(ctx->stream));
        for (int64_t s = 0; s < n; ++s) {
            const int32_t len = path_len[b + s];
            if (len < 1 || len > cap[b + s]) {
                gh_set_error("gh_text_viterbi: back-trace of string %lld ran past its bound", (long long)(b + s));
                return GH_ERR_INVALID;
            }
            GH_REQUIRE(written + len <= path_cap, "gh_text_viterbi: path_cap = %lld too small", (long long)path_cap);
            memcpy(path_rows + written, h_path.data() + h_path_off[s], (size_t)len * 4);
            written += len;
        }
    }
    ctx->last_chunks = (int)chunk_begin.size() - 1;
    return GH_OK;
}
