// spc_lesstate.hpp -- K9: spcpl.set_les_state (splib/spcpl.py:274-294) for a whole LES list in one launch, bit-identical
// to NumPy's legacy global generator (MT19937).  Included by spc_hip.hip inside its unnamed namespace.
//
// numpy.random.uniform(-1., 1., shape) takes two 32-bit MT19937 outputs a, b per element (C order) and returns
// -1.0 + 2.0 * (((a >> 5) * 67108864.0 + (b >> 6)) / 9007199254740992.0); set_les_state adds amp * r + prof[k] in float64
// (one rounding each, no FMA: this file is compiled with contraction off).  The LES take their words one after the other,
// U, V, THL, QT within one LES: LES l starts 8 * sum_{m<l} itot*jtot*ktot words after the start state (key, pos).
//
// MT19937 is serial, but linear over GF(2): with phi the characteristic polynomial (degree 19937) of the one-word step A
// and g_J = x^J mod phi, A^J = g_J(A) (Haramoto, Matsumoto, Nishimura, Panneton, L'Ecuyer, INFORMS J. Computing 20(3),
// 2008).  State S = key array at a twist boundary; A^i S is the window of 624 words starting i words into the stream
// generated from S, so g(A) S, word j = XOR over the set coefficients c_i of x[i + j]: one workgroup generates the
// 19937 + 623 words of S's stream in LDS and correlates them with g's coefficients (k_mt_jump).
//
// The launch splits the T generations (twists) it needs into K substreams of L generations; substream s starts from
// G_{sL} = A^{624 s L} G_0.  The starts come from ceil(log2 K) rounds of k_mt_jump: round b applies g_{624 L 2^b} to the
// starts whose index has bit b set, so the host derives ceil(log2 K) polynomials only.  k_les_state then twists each
// substream in LDS (three dependent phases), tempers, pairs words into doubles and writes the fields.  A jumped state is
// exact on the 19937 significant bits; the 31 low bits of key[0] are dead (the twist reads only the top bit of key[0]),
// and a jump leaves them arbitrary.  They are never output: a workgroup outputs only words it twisted (or, substream 0,
// the start state itself), and the final state is the generation the launch actually twisted last.

constexpr int MT_N = 624, MT_M = 397;
constexpr uint32_t MT_MATRIX_A = 0x9908b0dfu, MT_UPPER = 0x80000000u, MT_LOWER = 0x7fffffffu;
constexpr int MT_DEG = 19937;                                  // degree of phi
constexpr int MT_PW = (MT_DEG + 63) / 64;                      // 312 64-bit words: a polynomial of degree <= 19937
constexpr int MT_STREAM = MT_DEG + MT_N - 1;                   // words of S's stream the correlation reads
constexpr int MT_STREAM_GENS = (MT_STREAM + MT_N - 1) / MT_N;  // 33 generations of it in LDS (82 368 B)
constexpr int LS_THREADS = 256;

__host__ __device__ __forceinline__ uint32_t mt_mix(uint32_t k0, uint32_t k1, uint32_t km)
{
    const uint32_t y = (k0 & MT_UPPER) | (k1 & MT_LOWER);
    return km ^ (y >> 1) ^ ((0u - (y & 1u)) & MT_MATRIX_A);
}

__host__ __device__ __forceinline__ uint32_t mt_temper(uint32_t y)
{
    y ^= y >> 11;
    y ^= (y << 7) & 0x9d2c5680u;
    y ^= (y << 15) & 0xefc60000u;
    y ^= y >> 18;
    return y;
}

// ---- host: phi, x^J mod phi, the jump ---------------------------------------------------------------------------------
typedef std::vector<uint64_t> Gf2Poly;                         // bit i = coefficient of x^i, MT_PW words

// NumPy's twist (randomkit's mt19937_gen), in place
inline void mt_twist_host(uint32_t *key)
{
    int i = 0;
    for (; i < MT_N - MT_M; i++) key[i] = mt_mix(key[i], key[i + 1], key[i + MT_M]);
    for (; i < MT_N - 1; i++) key[i] = mt_mix(key[i], key[i + 1], key[i + MT_M - MT_N]);
    key[MT_N - 1] = mt_mix(key[MT_N - 1], key[0], key[MT_M - 1]);
}

// the stream x[0 .. n) generated from key (x[0 .. 623] = key; x[k + 624] = x[k + 397] ^ mix(x[k], x[k + 1]))
inline void mt_stream_host(const uint32_t *key, uint32_t *x, int64_t n)
{
    for (int64_t k = 0; k < n && k < MT_N; k++) x[k] = key[k];
    for (int64_t k = MT_N; k < n; k++) x[k] = mt_mix(x[k - MT_N], x[k - MT_N + 1], x[k - MT_N + MT_M]);
}

// phi by Berlekamp-Massey over GF(2) on bit 0 of x_1, x_2, ... (2 * 19937 words of the stream of init_genrand(5489)).
// Every nonzero output sequence of MT19937 has phi as its minimal polynomial (phi is primitive); degree checked.
inline const Gf2Poly &mt_phi()
{
    static Gf2Poly phi;
    static std::once_flag once;
    std::call_once(once, [] {
        const int n = 2 * MT_DEG;
        std::vector<uint32_t> key(MT_N), x(n + 1);
        key[0] = 5489u;
        for (int i = 1; i < MT_N; i++) key[i] = 1812433253u * (key[i - 1] ^ (key[i - 1] >> 30)) + (uint32_t)i;
        mt_stream_host(key.data(), x.data(), n + 1);
        const int W = (n + 64) / 64 + 2;
        std::vector<uint64_t> rs(W + 1, 0);                    // rs bit t = s_{n-1-t}: s reversed
        for (int t = 0; t < n; t++)
            if (x[1 + (n - 1 - t)] & 1u) rs[t >> 6] |= 1ull << (t & 63);
        std::vector<uint64_t> C(W, 0), B(W, 0), Tmp;
        C[0] = B[0] = 1;
        int L = 0, m = 1;
        for (int i = 0; i < n; i++) {
            // d = sum_{k=0..L} c_k s_{i-k} = parity(C & (rs >> (n-1-i)))
            const int off = n - 1 - i;
            uint64_t acc = 0;
            for (int w = 0; w <= L / 64; w++) {
                const int bit = off + 64 * w, q = bit >> 6, r = bit & 63;
                uint64_t v = rs[q] >> r;
                if (r) v |= rs[q + 1] << (64 - r);
                acc ^= C[w] & v;
            }
            if (!__builtin_parityll(acc)) { m++; continue; }
            Tmp = C;
            const int ws = m >> 6, bs = m & 63;
            for (int w = 0; w + ws < W; w++) {
                C[w + ws] ^= B[w] << bs;
                if (bs && w + ws + 1 < W) C[w + ws + 1] ^= B[w] >> (64 - bs);
            }
            if (2 * L <= i) { L = i + 1 - L; B = Tmp; m = 1; } else m++;
        }
        if (L != MT_DEG) { fprintf(stderr, "spc: Berlekamp-Massey gave degree %d, not %d\n", L, MT_DEG); abort(); }
        phi.assign(MT_PW, 0);                                  // phi_j = c_{L-j}
        for (int j = 0; j <= L; j++)
            if ((C[(L - j) >> 6] >> ((L - j) & 63)) & 1u) phi[j >> 6] |= 1ull << (j & 63);
    });
    return phi;
}

// r (2 * MT_PW words, degree < 2 * 19937) mod phi, into its low MT_PW words
inline void gf2_reduce(std::vector<uint64_t> &r)
{
    const Gf2Poly &phi = mt_phi();
    for (int i = 2 * MT_DEG - 2; i >= MT_DEG; i--) {
        if (!((r[i >> 6] >> (i & 63)) & 1u)) continue;
        const int s = i - MT_DEG, ws = s >> 6, bs = s & 63;
        for (int w = 0; w < MT_PW; w++) {
            const uint64_t v = phi[w];
            if (!v) continue;
            r[w + ws] ^= v << bs;
            if (bs) r[w + ws + 1] ^= v >> (64 - bs);
        }
    }
    r.resize(MT_PW);
}

inline uint64_t spread32(uint32_t v)
{
    uint64_t x = v;
    x = (x | (x << 16)) & 0x0000ffff0000ffffull;
    x = (x | (x << 8)) & 0x00ff00ff00ff00ffull;
    x = (x | (x << 4)) & 0x0f0f0f0f0f0f0f0full;
    x = (x | (x << 2)) & 0x3333333333333333ull;
    x = (x | (x << 1)) & 0x5555555555555555ull;
    return x;
}

inline Gf2Poly gf2_square(const Gf2Poly &a)
{
    std::vector<uint64_t> r(2 * MT_PW + 1, 0);
    for (int w = 0; w < MT_PW; w++) {
        r[2 * w] = spread32((uint32_t)a[w]);
        r[2 * w + 1] = spread32((uint32_t)(a[w] >> 32));
    }
    gf2_reduce(r);
    return r;
}

inline void gf2_mulx(Gf2Poly &a)
{
    uint64_t carry = 0;
    for (int w = 0; w < MT_PW; w++) {
        const uint64_t v = a[w];
        a[w] = (v << 1) | carry;
        carry = v >> 63;
    }
    if ((a[MT_DEG >> 6] >> (MT_DEG & 63)) & 1u) {
        const Gf2Poly &phi = mt_phi();
        for (int w = 0; w < MT_PW; w++) a[w] ^= phi[w];
    }
}

// x^J mod phi (cached: a launch of one geometry asks for the same few every time)
inline Gf2Poly mt_jump_poly(uint64_t J)
{
    static std::mutex mu;
    static std::map<uint64_t, Gf2Poly> cache;
    {
        std::lock_guard<std::mutex> g(mu);
        auto it = cache.find(J);
        if (it != cache.end()) return it->second;
        if (cache.size() > 256) cache.clear();
    }
    Gf2Poly r;
    const uint64_t half = J >> 1;
    bool have = false;
    {
        std::lock_guard<std::mutex> g(mu);
        auto it = cache.find(half);
        if (J > 1 && it != cache.end()) { r = it->second; have = true; }
    }
    if (have) {                                                // x^J = (x^(J/2))^2 [* x]
        r = gf2_square(r);
        if (J & 1) gf2_mulx(r);
    } else {
        r.assign(MT_PW, 0);
        r[0] = 1;
        for (int b = 63; b >= 0; b--) {
            if (!(J >> b)) continue;
            r = gf2_square(r);
            if ((J >> b) & 1) gf2_mulx(r);
        }
    }
    std::lock_guard<std::mutex> g(mu);
    cache.emplace(J, r);
    return r;
}

// g(A) S on the host: key_out[j] = XOR_{c_i = 1} x[i + j] over S's stream (key_out[0]'s 31 low bits are dead)
inline void mt_apply_poly_host(const Gf2Poly &g, const uint32_t *key, uint32_t *key_out)
{
    std::vector<uint32_t> x(MT_STREAM_GENS * MT_N);
    mt_stream_host(key, x.data(), (int64_t)x.size());
    std::vector<uint32_t> acc(MT_N, 0);
    for (int w = 0; w < MT_PW; w++) {
        uint64_t c = g[w];
        while (c) {
            const int i = 64 * w + __builtin_ctzll(c);
            c &= c - 1;
            const uint32_t *xi = x.data() + i;
            for (int j = 0; j < MT_N; j++) acc[j] ^= xi[j];
        }
    }
    memcpy(key_out, acc.data(), MT_N * sizeof(uint32_t));
}

// NumPy's state after drawing n words from (key_in, pos_in): (G_T, q - 624 T) with q = pos_in + n, T = (q - 1) div 624, or
// (key_in, q) when q <= 624.  G_T is one real twist of G_{T-1} = A^{624 (T-1)} G_0, so every bit of it is NumPy's (the
// twist reads only significant bits of G_{T-1}).
inline void mt_jump_host(const uint32_t *key_in, int64_t pos_in, int64_t n, uint32_t *key_out, int32_t *pos_out)
{
    const int64_t q = pos_in + n;
    std::vector<uint32_t> k(key_in, key_in + MT_N);
    if (q <= MT_N) {
        memcpy(key_out, k.data(), MT_N * sizeof(uint32_t));
        *pos_out = (int32_t)q;
        return;
    }
    const int64_t T = (q - 1) / MT_N;
    if (T > 1) mt_apply_poly_host(mt_jump_poly((uint64_t)MT_N * (uint64_t)(T - 1)), key_in, k.data());
    mt_twist_host(k.data());
    memcpy(key_out, k.data(), MT_N * sizeof(uint32_t));
    *pos_out = (int32_t)(q - MT_N * T);
}

// ---- device --------------------------------------------------------------------------------------------------------
// One round of the substream starts: state s (bit `bit` of s set) <- g(A) state s, where state s is still G_0 when no
// lower bit of s is set.  g is given as the ascending list of its set coefficients (uniform: scalar loads), so the
// correlation keeps LS_JUMP_UNROLL independent LDS reads per accumulator in flight instead of one per set bit.
constexpr int LS_JUMP_UNROLL = 8;
__global__ __launch_bounds__(LS_THREADS) void k_mt_jump(const uint32_t *__restrict__ key0, uint32_t *__restrict__ states,
                                                          const int32_t *__restrict__ coef, int32_t n_coef, int bit, int64_t K)
{
    __shared__ uint32_t x[MT_STREAM_GENS * MT_N];
    const int64_t s = blockIdx.x;
    if (s >= K || !((s >> bit) & 1)) return;
    const int t = threadIdx.x;
    const uint32_t *src = (s & ((int64_t(1) << bit) - 1)) ? states + s * MT_N : key0;
    for (int j = t; j < MT_N; j += LS_THREADS) x[j] = src[j];
    __syncthreads();
    for (int gen = 1; gen < MT_STREAM_GENS; gen++) {           // x[k + 624] = x[k + 397] ^ mix(x[k], x[k + 1]) in 3 phases
        uint32_t *o = x + (gen - 1) * MT_N;
        if (t < MT_N - MT_M) o[MT_N + t] = mt_mix(o[t], o[t + 1], o[t + MT_M]);                      // reads old words only
        __syncthreads();
        {
            const int j = t + (MT_N - MT_M);                                                           // 227 ... 453
            if (j < 2 * (MT_N - MT_M)) o[MT_N + j] = mt_mix(o[j], o[j + 1], o[j + MT_M]);              // new words 0 ... 226
        }
        __syncthreads();
        {
            const int j = t + 2 * (MT_N - MT_M);                                                       // 454 ... 623
            if (j < MT_N) o[MT_N + j] = mt_mix(o[j], o[j + 1], o[j + MT_M]);                           // new words 227 ... 396
        }
        __syncthreads();
    }
    uint32_t a0 = 0, a1 = 0, a2 = 0;
    const int j2 = t + 2 * LS_THREADS < MT_N ? t + 2 * LS_THREADS : MT_N - 1;
    int q = 0;
    for (; q + LS_JUMP_UNROLL <= n_coef; q += LS_JUMP_UNROLL) {
        int i[LS_JUMP_UNROLL];
#pragma unroll
        for (int u = 0; u < LS_JUMP_UNROLL; u++) i[u] = coef[q + u];        // 0 <= i < 19937: x[i + 623] is in LDS
#pragma unroll
        for (int u = 0; u < LS_JUMP_UNROLL; u++) {
            a0 ^= x[i[u] + t];
            a1 ^= x[i[u] + t + LS_THREADS];
            a2 ^= x[i[u] + j2];
        }
    }
    for (; q < n_coef; q++) {
        const int i = coef[q];
        a0 ^= x[i + t];
        a1 ^= x[i + t + LS_THREADS];
        a2 ^= x[i + j2];
    }
    uint32_t *dst = states + s * MT_N;
    dst[t] = a0;
    dst[t + LS_THREADS] = a1;
    if (t + 2 * LS_THREADS < MT_N) dst[t + 2 * LS_THREADS] = a2;
}

struct LsP {
    const uint32_t *key0;       // G_0 (the start state)
    const uint32_t *states;     // [K x 624] substream starts (state 0 unused)
    uint32_t *final_key;        // [624] G_T
    int64_t K, L, T;            // substreams, generations per substream, generations in all
    int64_t p, q;               // the launch draws words p ... q-1 (0 = G_0[0])
    const int64_t *elem_off;    // [n_les + 1]
    const int32_t *ktot;        // [n_les]
    int64_t n_les, pitch;
    const double *prof[4];
    double amp[4];
    double *out[4];
};

// Which LES a thread's current element belongs to, with what the element needs of it held in registers: a thread's elements
// only move forward, so the offset table and ktot are read again only when the element crosses into the next LES.
struct LsCursor {
    int64_t l;                  // -1 before the first element
    int64_t off, end4;          // elem_off[l]; 4 * elem_off[l + 1] (the first element of the next LES)
    uint32_t V, kt;             // elements per field, ktot
    int64_t row;                // l * pitch
};

__device__ __forceinline__ void ls_seek(const LsP &P, LsCursor &c, int64_t e)
{
    if (c.l >= 0 && e < c.end4) return;
    if (c.l < 0) {                                             // the first element of this workgroup: binary search
        int64_t lo_l = 0, hi_l = P.n_les - 1;
        while (lo_l < hi_l) {
            const int64_t mid = (lo_l + hi_l + 1) >> 1;
            if (4 * P.elem_off[mid] <= e) lo_l = mid; else hi_l = mid - 1;
        }
        c.l = lo_l;
    }
    while (4 * P.elem_off[c.l + 1] <= e) c.l++;                // e < 4 * elem_off[n_les]: stops at l <= n_les - 1
    c.off = P.elem_off[c.l];
    c.end4 = 4 * P.elem_off[c.l + 1];
    c.V = (uint32_t)(P.elem_off[c.l + 1] - c.off);
    c.kt = (uint32_t)P.ktot[c.l];
    c.row = c.l * P.pitch;
}

// the elements whose first word lies in generation `gen` (key array G in LDS)
__device__ __forceinline__ void ls_emit(const LsP &P, const uint32_t *G, int64_t gen, LsCursor &c)
{
    const int64_t base = (int64_t)MT_N * gen;
    int64_t lo = base > P.p ? base : P.p;
    if ((lo - P.p) & 1) lo++;
    const int64_t hi = base + MT_N < P.q ? base + MT_N : P.q;
    for (int64_t a = lo + 2 * (int64_t)threadIdx.x; a < hi; a += 2 * LS_THREADS) {
        const int j = (int)(a - base);
        const uint32_t wa = mt_temper(G[j]);
        const uint32_t wb = mt_temper(j + 1 < MT_N ? G[j + 1] : mt_mix(G[0], G[1], G[MT_M]));  // straddle: G_{gen+1}[0]
        const double d = ((double)(wa >> 5) * 67108864.0 + (double)(wb >> 6)) / 9007199254740992.0;
        const double r = -1.0 + 2.0 * d;
        const int64_t e = (a - P.p) >> 1;                      // element of the launch; LES l holds 4 * elem_off[l] ...
        ls_seek(P, c, e);
        const uint32_t el = (uint32_t)(e - 4 * c.off);         // < 4 V < 2^32
        const uint32_t f = el / c.V, idx = el - f * c.V;
        const uint32_t k = idx % c.kt;
        const double v = P.amp[f] * r;
        P.out[f][c.off + idx] = v + P.prof[f][c.row + k];
    }
}

__global__ __launch_bounds__(LS_THREADS) void k_les_state(LsP P)
{
    __shared__ uint32_t buf[2][MT_N];
    const int64_t s = blockIdx.x;
    const int t = threadIdx.x;
    const uint32_t *src = s == 0 ? P.key0 : P.states + s * MT_N;
    for (int j = t; j < MT_N; j += LS_THREADS) buf[0][j] = src[j];
    __syncthreads();
    LsCursor c;
    c.l = -1;
    c.off = c.end4 = c.row = 0;
    c.V = c.kt = 1;
    if (s == 0) ls_emit(P, buf[0], 0, c);                      // the prefix: words pos ... 623 of the start state
    int cur = 0;
    const int64_t g1 = s * P.L + P.L < P.T ? s * P.L + P.L : P.T;
    for (int64_t gen = s * P.L + 1; gen <= g1; gen++) {
        const uint32_t *o = buf[cur];
        uint32_t *nw = buf[cur ^ 1];
        if (t < MT_N - MT_M) nw[t] = mt_mix(o[t], o[t + 1], o[t + MT_M]);
        __syncthreads();
        {
            const int j = t + (MT_N - MT_M);
            if (j < 2 * (MT_N - MT_M)) nw[j] = mt_mix(o[j], o[j + 1], nw[j + MT_M - MT_N]);
        }
        __syncthreads();
        {
            const int j = t + 2 * (MT_N - MT_M);
            if (j < MT_N - 1) nw[j] = mt_mix(o[j], o[j + 1], nw[j + MT_M - MT_N]);
            else if (j == MT_N - 1) nw[j] = mt_mix(o[j], nw[0], nw[MT_M - 1]);
        }
        __syncthreads();
        cur ^= 1;
        ls_emit(P, buf[cur], gen, c);
        if (gen == P.T)
            for (int j = t; j < MT_N; j += LS_THREADS) P.final_key[j] = buf[cur][j];
    }
}

inline int64_t ls_align(int64_t b) { return (b + 255) / 256 * 256; }

// substreams: the host polynomials, the jump rounds and the generation; L chosen from a cost model of the two kernels
struct LsPlan {
    int64_t T, L, K;
    int rounds;
};

inline LsPlan ls_plan(int64_t n_words, int32_t pos_in, int64_t gens_per_substream, int cus)
{
    LsPlan pl;
    const int64_t q = pos_in + n_words;
    pl.T = q <= MT_N ? 0 : (q - 1) / MT_N;
    if (gens_per_substream > 0) {
        pl.L = gens_per_substream;
    } else {
        // a wave of k_mt_jump workgroups (one 82 KB workgroup per CU) is counted as 60 generations of one k_les_state
        // workgroup (a kernel trace puts it nearer 115: DESIGN.md section 7.2), and up to 8 k_les_state workgroups fit on a
        // CU: minimise rounds * waves * 60 + L over powers of two K
        const double JUMP_GENS = 60.0;
        int64_t best_L = pl.T > 0 ? pl.T : 1;
        double best = (double)best_L;
        for (int lk = 1; lk <= 20; lk++) {
            const int64_t K = int64_t(1) << lk;
            if (K > 8 * (int64_t)cus || K > pl.T) break;
            const int64_t L = (pl.T + K - 1) / K;
            const int64_t waves = (K / 2 + cus - 1) / cus;
            const double cost = lk * waves * JUMP_GENS + (double)L;
            if (cost < best) { best = cost; best_L = L; }
        }
        pl.L = best_L;
    }
    pl.K = pl.T > 0 ? (pl.T + pl.L - 1) / pl.L : 1;
    pl.rounds = 0;
    while ((int64_t(1) << pl.rounds) < pl.K) pl.rounds++;
    return pl;
}

// workspace: key0 [624] | final [624] | elem_off [n_les + 1] | ktot [n_les] | states [K x 624] | coefficient lists [rounds x 19937]
inline int64_t ls_workspace_bytes(int64_t n_les, const LsPlan &pl)
{
    return ls_align(2 * MT_N * 4) + ls_align((n_les + 1) * 8) + ls_align(n_les * 4) + ls_align(pl.K * MT_N * 4)
           + ls_align((int64_t)pl.rounds * MT_DEG * 4);
}
