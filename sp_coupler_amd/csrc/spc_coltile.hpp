// spc_coltile.hpp -- the LDS column tile of the kernels with a serial chain along k (K15, K17, K18, K21, K22, K23, K25), device
// and host side.  spc_hip.hip includes it twice: among the device headers before spc_diffuse.hpp (after spc_chain.hpp: SlabVec),
// and -- SPC_COLTILE_HOST defined -- after spc_launch.hpp (fail, ensure_lds, launch_status).
//
// Fields are [n_les][itot][jtot][ktot], C order, ktot contiguous.  A workgroup takes C consecutive columns of the flat column
// index, a contiguous run of C * ktot cells that may span rows i and LES (ColRun).  It brings the run into `tiles` LDS tiles,
// column c at c * pitch, each lane runs a serial chain along k in its own column, and the workgroup writes the run back.
//   pitch = (ktot + faces) | 1: ODD, so the lanes that work on the same k of their columns hit distinct banks (f32:
//           (pitch c + k) mod 32; f64: 2 (pitch c + k) mod 64, pairs of banks); faces = 1 where a column keeps its ktot + 1
//           faces in one row;
//   C     = the largest of 64 and 32 whose tiles fit MAX_LDS_BYTES (at least two workgroups per CU), else 16 where they fit the
//           whole HARD_LDS_BYTES (dynamic-LDS opt-in), else the ktot is unsupported (col_cols).
// A run travels between global memory and a tile by all lanes, coalesced: 16-byte accesses from the first 16-byte boundary on
// and single elements before it and after the last whole vector (col_split), so views off the 16-byte grid take the same path.
// col_move is that walk for a plain copy (K15, K25).  K18 and K21 compute on the way and keep their walks (rad_load, rad_store,
// hyd_load, hyd_store) on col_split and ColRun: one walker over a per-element functor was tried, and it changed the registers
// and the instruction mix of all four kernels.
#ifndef SPC_COLTILE_HOST

constexpr int DIF_STAGE = 2;                    // LES whose three profile rows a tile keeps in LDS behind its columns (K15, K25)

__host__ __device__ constexpr int col_pitch(int ktot, int faces) { return (ktot + faces) | 1; }

// the largest ktot of which 16 columns fit the LDS `tiles` times
inline int col_max_ktot(int esize, int tiles, int faces)
{
    int P = HARD_LDS_BYTES / (16 * tiles) / esize;
    if (!(P & 1)) --P;
    return P - faces;
}

// columns per workgroup of ktot levels of esize bytes, 0: unsupported
inline int col_cols(int ktot, int esize, int tiles, int faces)
{
    if (ktot < 1 || (esize != 4 && esize != 8) || ktot > col_max_ktot(esize, tiles, faces)) return 0;
    const int64_t col = (int64_t)tiles * col_pitch(ktot, faces) * esize;
    if (64 * col <= MAX_LDS_BYTES) return 64;
    if (32 * col <= MAX_LDS_BYTES) return 32;
    return 16;
}

// The run of workgroup `block`: nc columns from col0 on (the last tile is partial), len cells from cell `run` on; col0 is column
// rem0 of LES l0.  The order of the statements is the kernels' own from before the struct: their code is sensitive to it
// (tools/refactor_check.py).  K15 and K25 do not take it: they need l0 only behind their first copies and keep the 64-bit
// division there, with their three lines for col0 and nc.
struct ColRun {
    int64_t col0, l0, run;
    int nc, len;
    uint32_t rem0;
    __device__ __forceinline__ ColRun(const unsigned block, const int C, const int64_t ncols, const int nij, const int ktot)
    {
        col0 = (int64_t)block * C;
        const int64_t left = ncols - col0;
        nc = left < C ? (int)left : C;
        len = nc * ktot;
        l0 = col0 / nij;
        rem0 = (uint32_t)(col0 - l0 * nij);
        run = col0 * ktot;
    }
};

// where the vectors lie in a run of len elements that starts at g: head single elements, then nv whole vectors
template <typename T> __device__ __forceinline__ void col_split(const T *g, const int len, const int vec, int &head, int &nv)
{
    constexpr int V = 16 / (int)sizeof(T);
    if (!vec) {                                                     // the arrays lie differently on the grid: single elements
        head = len;
        nv = 0;
        return;
    }
    const int mis = (int)(((uintptr_t)g / sizeof(T)) % V);         // elements past a 16-byte boundary
    head = mis ? V - mis : 0;
    if (head > len) head = len;
    nv = (len - head) / V;
}

// the run g[0 ... len) <-> the tile (column c at c * P), by all THREADS lanes of the workgroup, UB vectors per lane and batch;
// STORE: tile -> g
template <typename T, int THREADS, int UB, bool STORE> __device__ __forceinline__ void col_move(T *g, T *tile, const int len, const int ktot, const int P)
{
    constexpr int V = 16 / (int)sizeof(T);
    using Vec = SlabVec<T, V>;
    const int tid = threadIdx.x;
    int head, nv;
    col_split<T>(g, len, 1, head, nv);
    const int tail0 = head + nv * V;
    // the elements before the first and after the last whole vector: fewer than 2 V
    {
        const int e = tid < head ? tid : tail0 + (tid - head);
        if (e < len) {
            const int c = e / ktot, k = e - c * ktot;
            if (STORE) g[e] = tile[c * P + k];
            else tile[c * P + k] = g[e];
        }
    }
    T *gv = g + head;
    for (int i0 = 0; i0 < nv; i0 += THREADS * UB) {
        Vec x[UB];
        if (!STORE) {
#pragma unroll
            for (int u = 0; u < UB; ++u) {
                const int i = i0 + u * THREADS + tid;
                if (i < nv) x[u] = *reinterpret_cast<const Vec *>(gv + (int64_t)i * V);
            }
        }
#pragma unroll
        for (int u = 0; u < UB; ++u) {
            const int i = i0 + u * THREADS + tid;
            if (i < nv) {
                const int e = head + i * V;
                int c = e / ktot, k = e - c * ktot;
#pragma unroll
                for (int v = 0; v < V; ++v) {
                    if (STORE) x[u].v[v] = tile[c * P + k];
                    else tile[c * P + k] = x[u].v[v];
                    if (++k == ktot) { k = 0; ++c; }
                }
                if (STORE) *reinterpret_cast<Vec *>(gv + (int64_t)i * V) = x[u];
            }
        }
    }
}

#else  // SPC_COLTILE_HOST ---------------------------------------------------------------------------------------------------

// the workgroups of C columns; `name`: the kernel's in the texts of spc_last_error()
static int col_grid(const char *name, int64_t ncols, int C, int64_t &grid)
{
    grid = (ncols + C - 1) / C;
    return grid > INT32_MAX ? fail(SPC_ERR_UNSUPPORTED, "%s: too many workgroups", name) : SPC_OK;
}

// f(std::integral_constant<int, C>) for the C that col_cols gave: a kernel template over C is launched from one place
template <typename F> static int col_dispatch(int C, F f)
{
    if (C == 64) return f(std::integral_constant<int, 64>());
    if (C == 32) return f(std::integral_constant<int, 32>());
    return f(std::integral_constant<int, 16>());
}

// The launch of a kernel with `tiles` tiles of C columns, one field per blockIdx.y, that stages profile rows behind them (K15, K25):
// p.stage = DIF_STAGE where the rows fit the budget of C behind the tiles, else 0.
template <typename T, typename K, typename P>
static int col_stage_launch(K kernel, const char *kernel_name, const char *name, P p, int C, int tiles, int n_fields, int threads, void *stream)
{
    const size_t tile = (size_t)tiles * C * col_pitch(p.ktot, 0) * sizeof(T), rows = (size_t)3 * DIF_STAGE * p.ktot * sizeof(T);
    p.stage = tile + rows <= (size_t)(C == 16 ? HARD_LDS_BYTES : MAX_LDS_BYTES) ? DIF_STAGE : 0;
    const size_t smem = tile + (p.stage ? rows : 0);
    int rc = ensure_lds(kernel, smem, kernel_name);
    if (rc) return rc;
    int64_t grid;
    if ((rc = col_grid(name, p.ncols, C, grid))) return rc;
    hipLaunchKernelGGL(kernel, dim3((unsigned)grid, (unsigned)n_fields), dim3(threads), smem, (hipStream_t)stream, p);
    return launch_status(kernel_name);
}

// Every written array wr[x] that is not nullptr against every array read, then against the written arrays before it (equal base
// pointers are what is detected: partially overlapping views are the caller's to avoid); bits: every pointer or'ed, for the
// alignment check that follows.
static int col_alias(const char *name, const void *const *in, int n_in, const void *const *wr, int n_wr, const char *const *wname, uintptr_t &bits)
{
    for (int x = 0; x < n_wr; ++x) {
        if (!wr[x]) continue;
        char who[64];                                                 // "<kernel>: <array>": fail() takes one string
        snprintf(who, sizeof(who), "%s: %s", name, wname[x]);
        for (int q = 0; q < n_in; ++q)
            if (in[q] == wr[x]) return fail(SPC_ERR_INVALID_ARGUMENT, "%s is also an input (it is written while they are read)", who);
        for (int q = 0; q < x; ++q)
            if (wr[q] == wr[x]) return fail(SPC_ERR_INVALID_ARGUMENT, "%s is the same array as another output", who);
        bits |= (uintptr_t)wr[x];
    }
    for (int q = 0; q < n_in; ++q) bits |= (uintptr_t)in[q];
    return SPC_OK;
}

#endif
