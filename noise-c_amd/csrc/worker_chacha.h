/*
 * worker_chacha.h — the resident worker's latency-first ChaChaPoly engine
 * (device code, included by worker.hip after chachapoly.hip): the quad-lane
 * ChaCha20, the Poly1305 tree, worker_chacha_fast for one-pass records and
 * worker_chacha_multi past them.  The text is the one worker.hip held; the
 * two record functions still carry their own block fetch, tree ladder and
 * tag finish (DESIGN.md section 8 says what sharing them measured).
 */
#ifndef NA_WORKER_CHACHA_H
#define NA_WORKER_CHACHA_H

namespace na {

/* ---------------------------------------------- latency-first ChaChaPoly
 *
 * One record on the whole workgroup, built for the depth of its dependency
 * chains rather than its instruction count (a lone wave issues about one
 * instruction per 4.7 cycles, so depth and count both cost time):
 *  - ChaCha20 four lanes per block (quad q = block q, lane c = column c:
 *    words c, 4+c, 8+c, 12+c), the diagonal rounds by quad DPP rotations of
 *    rows b, c, d: ~330 instructions per lane instead of ~1000;
 *  - Poly1305 one 16-byte block per lane (AD blocks, CT blocks, the length
 *    block: n of them), right-justified in N = 2^ceil(log2 n) lanes, and the
 *    polynomial sum_i b_i r^(n-i) as a left-aligned tree: level L sets
 *    v_j = v_j r^L + v_{j+L} for j = 0 mod 2L (in-wave shuffles below 64,
 *    LDS for 64 and 128), then * r: log2(n) multiplies deep;
 *  - open verifies first and writes plaintext only on a match.
 * Records of up to WFAST_BLOCKS - 1 units with n <= 256 take it
 * (worker_fast_fits), longer ones worker_chacha_multi; the result equals
 * seal_il / open_il's bit for bit (the same Poly1305 value:
 * sum_i b_i r^(n-i+1) mod 2^130-5 + s). */
constexpr uint32_t WFAST_BLOCKS = 64; /* ChaCha blocks: 4 lanes each on 256 threads */

NA_DEV bool worker_fast_fits(uint32_t len, uint32_t ad_len)
{
    const uint32_t blocks = (len + 63) / 64 + 1;
    const uint32_t n = (ad_len + 15) / 16 + (len + 15) / 16 + 1;
    return blocks <= WFAST_BLOCKS && n <= 256;
}

template <int CTRL>
NA_DEV uint32_t quad_perm(uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xf, 0xf, false); }

/* quad_perm controls: lane i of a quad reads lane perm[i] */
constexpr int QP_NEXT1 = 0x39; /* [1,2,3,0] */
constexpr int QP_NEXT2 = 0x4e; /* [2,3,0,1] */
constexpr int QP_NEXT3 = 0x93; /* [3,0,1,2] */

/* ChaCha20 block `ctr` on the four lanes of a quad; lane c returns words
   c, 4+c, 8+c, 12+c of the key stream (chacha.c:74-133 layout). */
NA_DEV void chacha_quad(const uint32_t key[8], uint32_t ctr, uint32_t n_lo, uint32_t n_hi, int c,
                        uint32_t &oa, uint32_t &ob, uint32_t &oc, uint32_t &od)
{
    const uint32_t a0 = c == 0 ? 0x61707865u : c == 1 ? 0x3320646eu : c == 2 ? 0x79622d32u : 0x6b206574u;
    const uint32_t b0 = c == 0 ? key[0] : c == 1 ? key[1] : c == 2 ? key[2] : key[3];
    const uint32_t c0 = c == 0 ? key[4] : c == 1 ? key[5] : c == 2 ? key[6] : key[7];
    const uint32_t d0 = c == 0 ? ctr : c == 1 ? 0u : c == 2 ? n_lo : n_hi;
    uint32_t a = a0, b = b0, cc = c0, d = d0;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        NA_QR(a, b, cc, d);                                   /* columns */
        b = quad_perm<QP_NEXT1>(b); cc = quad_perm<QP_NEXT2>(cc); d = quad_perm<QP_NEXT3>(d);
        NA_QR(a, b, cc, d);                                   /* diagonals */
        b = quad_perm<QP_NEXT3>(b); cc = quad_perm<QP_NEXT2>(cc); d = quad_perm<QP_NEXT1>(d);
    }
    oa = a + a0; ob = b + b0; oc = cc + c0; od = d + d0;
}

/* chacha_quad for two blocks at once (blocks ctr0 and ctr1 on the same
   quad): two independent dependency chains in one instruction stream, so a
   lone wave's issue slots fill with the other block's work (the multi-pass
   records' passes, two per step) */
NA_DEV void chacha_quad_x2(const uint32_t key[8], uint32_t ctr0, uint32_t ctr1, uint32_t n_lo, uint32_t n_hi,
                           int c, uint32_t o0[4], uint32_t o1[4])
{
    const uint32_t a0 = c == 0 ? 0x61707865u : c == 1 ? 0x3320646eu : c == 2 ? 0x79622d32u : 0x6b206574u;
    const uint32_t b0 = c == 0 ? key[0] : c == 1 ? key[1] : c == 2 ? key[2] : key[3];
    const uint32_t c0 = c == 0 ? key[4] : c == 1 ? key[5] : c == 2 ? key[6] : key[7];
    const uint32_t d0 = c == 0 ? ctr0 : c == 1 ? 0u : c == 2 ? n_lo : n_hi;
    const uint32_t d1 = c == 0 ? ctr1 : d0;
    uint32_t a = a0, b = b0, cc = c0, d = d0;
    uint32_t e = a0, f = b0, g = c0, h = d1;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        NA_QR(a, b, cc, d);
        NA_QR(e, f, g, h);
        b = quad_perm<QP_NEXT1>(b); cc = quad_perm<QP_NEXT2>(cc); d = quad_perm<QP_NEXT3>(d);
        f = quad_perm<QP_NEXT1>(f); g = quad_perm<QP_NEXT2>(g); h = quad_perm<QP_NEXT3>(h);
        NA_QR(a, b, cc, d);
        NA_QR(e, f, g, h);
        b = quad_perm<QP_NEXT3>(b); cc = quad_perm<QP_NEXT2>(cc); d = quad_perm<QP_NEXT1>(d);
        f = quad_perm<QP_NEXT3>(f); g = quad_perm<QP_NEXT2>(g); h = quad_perm<QP_NEXT1>(h);
    }
    o0[0] = a + a0; o0[1] = b + b0; o0[2] = cc + c0; o0[3] = d + d0;
    o1[0] = e + a0; o1[1] = f + b0; o1[2] = g + c0; o1[3] = h + d1;
}

/* 16 bytes at p (16-B aligned LDS), bytes from `n` on cleared */
NA_DEV void lds_block(const uint8_t *p, uint32_t n, uint32_t w[4])
{
    const uint4 v = *(const uint4 *)p;
    w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int rem = (int)n - 4 * i;
        w[i] &= rem >= 4 ? 0xffffffffu : (rem <= 0 ? 0u : ((1u << (8 * rem)) - 1u));
    }
}

struct FastLds {
    uint32_t dbg[8];         /* s_memtime stamps of thread 0 (debug hook) */
    uint32_t rs[8];          /* r, s (key stream words 0..7 of block 0) */
    uint32_t v[4][5];        /* the tree's cross-wave partners (levels 64, 128) */
    uint32_t verdict;
};

/* v of lane t + L (the tree's partner) for L < 64: DPP where the partner is
   in the same row of 16 lanes, a lane shuffle otherwise */
template <uint32_t L>
NA_DEV uint32_t from_plus(uint32_t x, int lane)
{
    if constexpr (L == 1) return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0xb1, 0xf, 0xf, false);  /* quad [1,0,3,2] */
    else if constexpr (L == 2) return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x4e, 0xf, 0xf, false); /* quad [2,3,0,1] */
    else if constexpr (L == 4) return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x104, 0xf, 0xf, false); /* row_shl:4 */
    else if constexpr (L == 8) return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x108, 0xf, 0xf, false); /* row_shl:8 */
    else return (uint32_t)__shfl((int)x, lane + (int)L, 64);
}

/* One level of the Poly1305 tree: lanes j = 0 mod 2L set v_j = v_j r^L + v_{j+L};
   mP holds r^L on entry and r^(2L) on exit (when a next level exists). */
template <uint32_t L>
NA_DEV void tree_level(Fe &v, Mul &mP, int t, uint32_t N, FastLds &F)
{
    if (L >= N) return; /* uniform */
    const int lane = t & 63;
    Fe w;
    if constexpr (L < 64) {
        w.l0 = from_plus<L>(v.l0, lane);
        w.l1 = from_plus<L>(v.l1, lane);
        w.l2 = from_plus<L>(v.l2, lane);
        w.l3 = from_plus<L>(v.l3, lane);
        w.l4 = from_plus<L>(v.l4, lane);
    } else {
        /* partner t + L sits in another wave: through LDS */
        if (lane == 0 && (t & (int)(2 * L - 1)) == (int)L) {
            const int slot = t >> 6;
            F.v[slot][0] = v.l0; F.v[slot][1] = v.l1; F.v[slot][2] = v.l2;
            F.v[slot][3] = v.l3; F.v[slot][4] = v.l4;
        }
        __syncthreads();
        const int slot = min((t + (int)L) >> 6, 3); /* receivers: 1, 2 or 3 */
        w = Fe{F.v[slot][0], F.v[slot][1], F.v[slot][2], F.v[slot][3], F.v[slot][4]};
        __syncthreads();
    }
    const Mul cur = mP;
    if (2 * L < N) mP = mk_mul(fe_mul(mul_fe(cur), cur)); /* r^(2L), off the chain */
    if ((t & (int)(2 * L - 1)) == 0) v = fe_carry(fe_add(fe_mul(v, cur), w));
}

/* rec: len bytes (+ the tag for open) in LDS, 16-B aligned; ad: ad_len bytes
   (16-B aligned, padded).  256 threads, every one calls this. */
template <bool OPEN>
NA_DEV bool worker_chacha_fast(uint8_t *rec, const uint8_t *ad, uint32_t ad_len, uint32_t len,
                               const uint8_t *key8, uint64_t nonce, FastLds &F)
{
    const int t = (int)threadIdx.x, c = t & 3;
    const uint32_t q = (uint32_t)t >> 2; /* ChaCha block */
    const uint64_t c00 = __builtin_amdgcn_s_memtime();
#define NA_FSTAMP(k) do { if (t == 0) F.dbg[k] = (uint32_t)(__builtin_amdgcn_s_memtime() - c00); } while (0)
    uint32_t key[8];
    load_key(key8, key);
    const uint32_t n_lo = (uint32_t)nonce, n_hi = (uint32_t)(nonce >> 32);
    const uint32_t J = (len + 63) / 64; /* data blocks 1..J */
    uint32_t ks[4] = {0, 0, 0, 0};
    if (q <= J) chacha_quad(key, q, n_lo, n_hi, c, ks[0], ks[1], ks[2], ks[3]);
    if (q == 0) { F.rs[c] = ks[0]; F.rs[4 + c] = ks[1]; }
    NA_FSTAMP(0); /* ChaCha done (thread 0's quad) */
    /* data words 64(q-1) + 4c + 16i, i = 0..3: key stream word 4i + c */
    uint32_t pt[4] = {0, 0, 0, 0};
    if (q >= 1 && q <= J) {
        uint32_t *w = (uint32_t *)(rec + 64 * (q - 1) + 4 * c);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            pt[i] = w[4 * i] ^ ks[i];
            if (!OPEN) w[4 * i] = pt[i]; /* CT; bytes past len are overwritten by the tag */
        }
    }
    __syncthreads();
    NA_FSTAMP(1); /* CT in LDS, r and s published */
    /* Poly1305 block of this lane, right-justified in N lanes */
    const uint32_t a = (ad_len + 15) / 16, m = (len + 15) / 16, n = a + m + 1;
    const uint32_t N = n <= 1 ? 1u : 1u << (32 - __builtin_clz(n - 1));
    const int i = t - (int)(N - n);
    Fe v = fe_zero();
    if (i >= 0 && (uint32_t)i < n) {
        uint32_t b[4];
        if ((uint32_t)i < a) {
            lds_block(ad + 16 * i, ad_len - 16 * i, b);
        } else if ((uint32_t)i < a + m) {
            const uint32_t j = (uint32_t)i - a;
            lds_block(rec + 16 * j, len - 16 * j, b);
        } else {
            b[0] = ad_len; b[1] = 0; b[2] = len; b[3] = 0;
        }
        fe_add_block(v, b[0], b[1], b[2], b[3]);
    }
    const Fe r = fe_clamp_r(F.rs[0], F.rs[1], F.rs[2], F.rs[3]);
    Mul mP = mk_mul(r); /* r^L */
    NA_FSTAMP(2); /* Poly block loaded */
    /* levels 1..8 by DPP (quad swaps, row shifts), 16 and 32 by lane
       shuffles, 64 and 128 through LDS; each level a uniform branch on N */
    tree_level<1>(v, mP, t, N, F);
    tree_level<2>(v, mP, t, N, F);
    tree_level<4>(v, mP, t, N, F);
    tree_level<8>(v, mP, t, N, F);
    tree_level<16>(v, mP, t, N, F);
    tree_level<32>(v, mP, t, N, F);
    tree_level<64>(v, mP, t, N, F);
    tree_level<128>(v, mP, t, N, F);
    NA_FSTAMP(3); /* tree done */
    /* thread 0: the tag; every lane of the group got the same tree, so
       only thread 0's value is the sum */
    if (t == 0) {
        v = fe_mul(v, mk_mul(r));
        const uint32_t s[4] = {F.rs[4], F.rs[5], F.rs[6], F.rs[7]};
        uint32_t tag[4];
        fe_finish(v, s, tag);
        if (OPEN) {
            uint32_t got[4];
            load16(rec + len, 16, got);
            F.verdict = tag_equal(tag, got) ? 1u : 0u;
        } else {
            store16(rec + len, 16, tag);
        }
    }
    NA_FSTAMP(4); /* tag */
    if (!OPEN) return true;
    __syncthreads();
    const bool ok = F.verdict != 0;
    if (ok && q >= 1 && q <= J) {
        uint32_t *w = (uint32_t *)(rec + 64 * (q - 1) + 4 * c);
#pragma unroll
        for (int i2 = 0; i2 < 4; ++i2) w[4 * i2] = pt[i2]; /* bytes past len: not copied out */
    }
    NA_FSTAMP(5);
#undef NA_FSTAMP
    return ok;
}

/* Records past one pass (more than 63 units, or a Poly1305 input of more
   than 256 blocks): the same layout over P = ceil((J + 1) / 64) ChaCha
   passes, and G = ceil(n / 256) Poly1305 blocks per lane — lane j runs
   Horner with r over its G consecutive blocks (right-justified chunks),
   then the tree of worker_chacha_fast sums the chunks with unit R = r^G:
     poly = (sum_j h_j R^(NL-1-j)) r,  h_j = sum_k b_(jG+k-pad) r^(G-1-k),
   which is sum_i b_i r^(n-i+1) again.  Seal XORs each pass into the record
   in LDS, then authenticates the ciphertext; open authenticates first (pass
   0 for r and s) and decrypts only a verified record.  A separate
   instantiation, so records of one pass keep worker_chacha_fast unchanged
   (round 3 measured a merged version costing them 0.3-0.8 us). */
/* XOR the key stream of blocks 1..J into the record in LDS: pass p holds
   blocks 64p + q (pass 0's key stream, ks0, computed already); the other
   passes two at a time (chacha_quad_x2) */
NA_DEV void multi_xor_one(uint8_t *rec, uint32_t v, uint32_t J, int c, const uint32_t ks[4])
{
    if (v >= 1 && v <= J) {
        uint32_t *w = (uint32_t *)(rec + 64 * (v - 1) + 4 * c);
#pragma unroll
        for (int i = 0; i < 4; ++i) w[4 * i] ^= ks[i];
    }
}

NA_DEV void multi_xor_passes(uint8_t *rec, const uint32_t key[8], uint32_t n_lo, uint32_t n_hi, int c, uint32_t q,
                             uint32_t J, uint32_t P, const uint32_t ks0[4])
{
    multi_xor_one(rec, q, J, c, ks0);
    for (uint32_t p = 1; p < P; p += 2) {
        const uint32_t v0 = 64 * p + q, v1 = v0 + 64;
        uint32_t k0[4], k1[4];
        if (p + 1 < P) { /* uniform */
            chacha_quad_x2(key, v0, v1, n_lo, n_hi, c, k0, k1);
            multi_xor_one(rec, v0, J, c, k0);
            multi_xor_one(rec, v1, J, c, k1);
        } else {
            chacha_quad(key, v0, n_lo, n_hi, c, k0[0], k0[1], k0[2], k0[3]);
            multi_xor_one(rec, v0, J, c, k0);
        }
    }
}

template <bool OPEN>
NA_DEV bool worker_chacha_multi(uint8_t *rec, const uint8_t *ad, uint32_t ad_len, uint32_t len,
                                const uint8_t *key8, uint64_t nonce, FastLds &F)
{
    const int t = (int)threadIdx.x, c = t & 3;
    const uint32_t q = (uint32_t)t >> 2;
    const uint64_t c00 = __builtin_amdgcn_s_memtime();
#define NA_FSTAMP(k) do { if (t == 0) F.dbg[k] = (uint32_t)(__builtin_amdgcn_s_memtime() - c00); } while (0)
    uint32_t key[8];
    load_key(key8, key);
    const uint32_t n_lo = (uint32_t)nonce, n_hi = (uint32_t)(nonce >> 32);
    const uint32_t J = (len + 63) / 64, P = (J + 1 + 63) / 64; /* blocks 0..J in P passes */
    /* ChaCha pass p: block v = 64p + q; data words 64(v-1) + 4c + 16i */
    uint32_t ks0[4] = {0, 0, 0, 0}; /* pass 0 (open: XORed after the verdict) */
    chacha_quad(key, q, n_lo, n_hi, c, ks0[0], ks0[1], ks0[2], ks0[3]);
    if (q == 0) { F.rs[c] = ks0[0]; F.rs[4 + c] = ks0[1]; }
    if (!OPEN) multi_xor_passes(rec, key, n_lo, n_hi, c, q, J, P, ks0); /* CT; bytes past len: the tag overwrites */
    __syncthreads();
    NA_FSTAMP(0); /* seal: CT in LDS; both: r and s published */
    const uint32_t a = (ad_len + 15) / 16, m = (len + 15) / 16, n = a + m + 1;
    const uint32_t G = (n + 255) / 256, NL = (n + G - 1) / G, pad = NL * G - n;
    const uint32_t N = NL <= 1 ? 1u : 1u << (32 - __builtin_clz(NL - 1));
    const int j = t - (int)(N - NL); /* this lane's chunk */
    const Fe r = fe_clamp_r(F.rs[0], F.rs[1], F.rs[2], F.rs[3]);
    const Mul mr = mk_mul(r);
    Fe h = fe_zero();
    if (j >= 0 && (uint32_t)j < NL) {
        for (uint32_t k = 0; k < G; ++k) {
            const int idx = j * (int)G + (int)k - (int)pad; /* 0-based block of the Poly input */
            if (idx < 0) continue;                          /* leading padding of chunk 0 */
            uint32_t b[4];
            const uint32_t i = (uint32_t)idx;
            if (i < a) {
                lds_block(ad + 16 * i, ad_len - 16 * i, b);
            } else if (i < a + m) {
                const uint32_t jj = i - a;
                lds_block(rec + 16 * jj, len - 16 * jj, b);
            } else {
                b[0] = ad_len; b[1] = 0; b[2] = len; b[3] = 0;
            }
            h = fe_mul(h, mr);
            fe_add_block(h, b[0], b[1], b[2], b[3]);
        }
    }
    NA_FSTAMP(1); /* chunks' Horner done */
    /* R = r^G (G <= 17), square-and-multiply, the same in every lane */
    Fe R = r;
    {
        const int top = 31 - __builtin_clz(G);
        for (int bit = top - 1; bit >= 0; --bit) {
            R = fe_mul(R, mk_mul(R));
            if ((G >> bit) & 1u) R = fe_mul(R, mr);
        }
    }
    Mul mP = mk_mul(R);
    Fe vv = h;
    tree_level<1>(vv, mP, t, N, F);
    tree_level<2>(vv, mP, t, N, F);
    tree_level<4>(vv, mP, t, N, F);
    tree_level<8>(vv, mP, t, N, F);
    tree_level<16>(vv, mP, t, N, F);
    tree_level<32>(vv, mP, t, N, F);
    tree_level<64>(vv, mP, t, N, F);
    tree_level<128>(vv, mP, t, N, F);
    NA_FSTAMP(2); /* tree done */
    if (t == 0) {
        vv = fe_mul(vv, mr);
        const uint32_t s[4] = {F.rs[4], F.rs[5], F.rs[6], F.rs[7]};
        uint32_t tag[4];
        fe_finish(vv, s, tag);
        if (OPEN) {
            uint32_t got[4];
            load16(rec + len, 16, got);
            F.verdict = tag_equal(tag, got) ? 1u : 0u;
        } else {
            store16(rec + len, 16, tag);
        }
    }
    NA_FSTAMP(3); /* tag */
    if (!OPEN) return true;
    __syncthreads();
    const bool ok = F.verdict != 0;
    if (ok) multi_xor_passes(rec, key, n_lo, n_hi, c, q, J, P, ks0); /* decrypt the verified record in LDS */
    NA_FSTAMP(4);
#undef NA_FSTAMP
    return ok;
}

} // namespace na

#endif
