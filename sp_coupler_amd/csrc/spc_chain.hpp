// spc_chain.hpp -- the slab chain of the kernels that reduce or update the LES 3-D fields along (i, j) per (LES, level) (K10, K11,
// K12, K14, K20), device and host side.  spc_hip.hip includes it twice: among the device headers before spc_slab.hpp, and --
// SPC_CHAIN_HOST defined -- after spc_launch.hpp (fail), ahead of the host sides of the five.
//
// Fields are [n_les][itot][jtot][ktot], C order, ktot contiguous, 64-bit element offsets.  A lane owns V adjacent levels of one
// LES (V = 16 B / sizeof(T) where every pointer, ktot and every pitch lie on the 16-byte grid, else 1), consecutive lanes
// consecutive k, and walks the nij = itot * jtot rows in row-major order: NumPy's sequential sum acc = +0.0; acc += x fixes that
// chain.  Its mean is one IEEE division by T(nij).  The walks themselves, and the zero of K11, K12 and K14, stay in the kernels:
// what was tried and what it did to their code is in DESIGN.md 7.5.
#ifndef SPC_CHAIN_HOST

template <typename T, int V> struct alignas(sizeof(T) * V) SlabVec {
    T v[V];
};

// lane g of a launch of n_les * (ktot / V) lanes per field
template <int V> struct ChainLane {
    int64_t l;                     // its LES
    int k;                         // the first of its V levels
    __device__ __forceinline__ ChainLane(const int64_t g, const int ktot)
    {
        const int kv = ktot / V;
        l = g / kv;
        k = (int)(g - l * kv) * V;
    }
    // its levels in row 0 of its LES: the element offset, and the place in a field
    __device__ __forceinline__ int64_t cell(const int nij, const int64_t ktot) const { return l * nij * ktot + k; }
    template <typename E> __device__ __forceinline__ E *cell(E *field, const int nij, const int64_t ktot) const { return field + l * nij * ktot + k; }
    // ... and in a profile or a mean [n_les][pitch]
    __device__ __forceinline__ int64_t row(const int64_t pitch) const { return l * pitch + k; }
    template <typename E> __device__ __forceinline__ E *row(E *prof, const int64_t pitch) const { return prof + l * pitch + k; }
};

// numpy starts a sum from add's identity: a plane of -0.0 sums to +0.0.  (K10 and K20; the lanes of K11, K12 and K14 zero their
// several sums level by level in a loop of their own: through a function their 16-byte forms allocate other registers)
template <typename T, int V> __device__ __forceinline__ void chain_zero(SlabVec<T, V> &acc)
{
#pragma unroll
    for (int v = 0; v < V; ++v) acc.v[v] = (T)0;
}

// The sum over cnt rows becomes their mean, in place: IEEE division (the build has no fast-math).  Returns acc, for the store that
// follows: `*place = chain_mean(acc, cnt)` divides before it forms the place, as the kernels did.
template <typename T, int V> __device__ __forceinline__ SlabVec<T, V> &chain_mean(SlabVec<T, V> &acc, const T cnt)
{
#pragma unroll
    for (int v = 0; v < V; ++v) acc.v[v] = acc.v[v] / cnt;
    return acc;
}

#else  // SPC_CHAIN_HOST -----------------------------------------------------------------------------------------------------

template <typename T> constexpr int CHAIN_V = 16 / (int)sizeof(T);    // the levels of a lane with 16-byte accesses

// the kernel's text `fmt` ("%s<name>: ... %lld ... %lld") where pitch a or pitch b is smaller than ktot
static int chain_pitch(int32_t ktot, int64_t a, int64_t b, const char *fmt)
{
    return a < ktot || b < ktot ? fail(SPC_ERR_INVALID_ARGUMENT, fmt, "", (long long)a, (long long)b) : SPC_OK;
}

// Every written array wr[x] that is not nullptr against every array read, then against the written arrays before it (equal base
// pointers are what is detected: partially overlapping views are the caller's to avoid), with the kernel's own two texts.
static int chain_alias(const void *const *in, int n_in, const void *const *wr, int n_wr, const char *also_input, const char *same)
{
    for (int x = 0; x < n_wr; ++x) {
        if (!wr[x]) continue;
        for (int q = 0; q < n_in; ++q)
            if (wr[x] == in[q]) return fail(SPC_ERR_INVALID_ARGUMENT, "%s", also_input);
        for (int q = 0; q < x; ++q)
            if (wr[x] == wr[q]) return fail(SPC_ERR_INVALID_ARGUMENT, "%s", same);
    }
    return SPC_OK;
}

// The launch of a chain kernel: wide (V = CHAIN_V, else 1), chains = n_les * (ktot / V) lanes per field or job, grid workgroups of
// `threads` lanes.  bits: every pointer a lane reaches with V elements at once, ktot and the pitches in bytes, or'ed; single: the
// pointers it reads one element at a time.  Refuses, in this order: a pointer off the grid of T; ktot == 1 with the kernel's text
// `one_level` (nullptr: the kernel takes it); more than 2^31 - 1 workgroups.  narrow: the kernel wants V = 1 whatever the bits say.
template <typename T>
static int chain_geometry(const char *name, uintptr_t bits, uintptr_t single, int64_t n_les, int32_t ktot, int threads, const char *one_level,
                          bool &wide, int64_t &chains, int64_t &grid, bool narrow = false)
{
    if ((bits | single) % sizeof(T)) return fail(SPC_ERR_INVALID_ARGUMENT, "%s: a pointer is not aligned to its element type", name);
    if (one_level && ktot == 1) return fail(SPC_ERR_UNSUPPORTED, "%s", one_level);
    wide = bits % 16 == 0 && !narrow;                 // every row of every array starts on a 16-byte boundary
    chains = n_les * (int64_t)(wide ? ktot / CHAIN_V<T> : ktot);
    grid = (chains + threads - 1) / threads;
    return grid > INT32_MAX ? fail(SPC_ERR_UNSUPPORTED, "%s: too many workgroups", name) : SPC_OK;
}

#endif
