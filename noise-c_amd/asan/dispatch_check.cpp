/*
 * dispatch_check.cpp — SANITIZER TEST HARNESS ONLY
 * (make -C noise-c_amd dispatch_check; tests/test_dispatch_host.py).
 *
 * Kernel choice and job checks (csrc/dispatch.h) run on the CPU under
 * ASan/UBSan, over never-dereferenced pointers.
 *
 *   dispatch_check           the job checks: the argument and independence
 *                            cases of tests/test_abi.py, pointer / stride /
 *                            count values at the arithmetic edges, and every
 *                            small job (n <= 8, len <= 48) against a brute-force
 *                            "do any two records meet"
 *   dispatch_check --table   one line per case: the job, the launches it
 *                            plans (plan_print) and its return code, for
 *                            tests/golden/dispatch_plans.txt.gz
 *   dispatch_check --table G only environment group G of the table
 *   dispatch_check --groups  the groups' environment settings
 *   dispatch_check --duplex-ragged
 *                            plan_duplex_ragged against plan_ragged over both
 *                            ciphers, record counts, lanes and flags per job,
 *                            the NOISE_AEAD_RAGGED_DUPLEX switch and the
 *                            segmented kernel's occupancy, and
 *                            check_duplex_ragged at the span edges
 *                            (tests/test_dispatch_duplex_ragged_host.py)
 *
 * The golden table was recorded from the selection code as it stood before
 * dispatch.h existed, compiled with its launches replaced by prints: this
 * file built with DISPATCH_CHECK_BACKEND naming a header takes the six
 * backend_* functions below from it (there: the old library's entry points,
 * one process per environment group), so both sides enumerate the same cases.
 */
#include "../csrc/dispatch.h"

#include <cinttypes>
#include <vector>

using namespace na;

enum { CHACHA = NOISE_CIPHER_CHACHAPOLY, AES = NOISE_CIPHER_AESGCM };

/* an environment group: one switch at one value, the others at their defaults */
struct EnvGroup { const char *name, *value; };
static const EnvGroup GROUPS[] = {
    {nullptr, nullptr},
    {"NOISE_AEAD_SOLO", "0"},
    {"NOISE_AEAD_SEG", "0"},
    {"NOISE_AEAD_SEG", "2"},
    {"NOISE_AEAD_CT_GHASH", "1"},
    {"NOISE_AEAD_LANES", "narrow"},
    {"NOISE_AEAD_DUPLEX_RUNS", "0"},
    {"NOISE_AEAD_GCM_SHAPE", "w1024r1"},
    {"NOISE_AEAD_GCM_SHAPE", "w1024r2"},
    {"NOISE_AEAD_GCM_SHAPE", "w1024r2k8"},
    {"NOISE_AEAD_GCM_DUPLEX", "staged"},
};
constexpr int N_GROUPS = sizeof GROUPS / sizeof GROUPS[0];

static bool g_quiet; /* the checks run the backend without printing */

#ifdef DISPATCH_CHECK_BACKEND
#include DISPATCH_CHECK_BACKEND
#else
/* The entry points' flow (aead_api.hip run_uniform / run_duplex / run_ragged)
   over dispatch.h: check, plan, and print the plan where they would launch. */
static Switches g_sw;
static uint32_t g_cus, g_resident;

static void backend_group(const EnvGroup &g)
{
    for (const EnvGroup &o : GROUPS)
        if (o.name) unsetenv(o.name);
    if (g.name) setenv(g.name, g.value, 1);
    g_sw = switches_from_env();
}

/* the device: its CU count, and the segmented kernel's resident workgroups */
static void backend_device(uint32_t cus, uint32_t resident) { g_cus = cus, g_resident = resident; }

static int launched(const Plan &p)
{
    char line[256];
    if (p.rc || !p.grid) return p.rc;
    plan_print(p, line, sizeof line);
    if (!g_quiet) printf(" | %s", line);
    return NOISE_ERROR_NONE;
}

static int backend_uniform(int cipher, const NoiseAeadUniform *j, bool open)
{
    const int rc = check_uniform(j, open);
    return rc ? rc : launched(plan_uniform(cipher, j, open, g_sw, cipher == CHACHA ? g_cus : 0));
}

static int backend_duplex(int cipher, const NoiseAeadUniform *sj, const NoiseAeadUniform *oj)
{
    int rc = check_duplex(sj, oj);
    if (rc) return rc;
    const Plan p = plan_duplex(cipher, sj, oj, g_sw, cipher == CHACHA ? g_cus : 0);
    if (p.shared) return launched(p);
    rc = backend_uniform(cipher, sj, false);
    return rc ? rc : backend_uniform(cipher, oj, true);
}

static int backend_ragged(int cipher, const NoiseAeadRagged *j, bool open)
{
    const int rc = check_ragged(j);
    if (rc) return rc;
    return launched(plan_ragged(cipher, j, open, g_sw, ragged_takes_seg(cipher, j, g_sw) ? g_resident : 0));
}

/* which = 0 noise_aead_dev_default_lanes, 1 _duplex_lanes, 2 na_chacha_lanes, 3 na_aes_lanes */
static int backend_lanes(int which, int cipher, uint32_t n, uint32_t max_len)
{
    if (which == 2) return (int)host_chacha_lanes(n, max_len, g_sw);
    if (which == 3) return (int)host_aes_lanes(g_sw);
    if (cipher == AES) return (int)PLAN_GCM_LANES;
    return chacha_uniform_lanes(0, n, true, which == 1, g_sw);
}
#endif

/* ------------------------------------------------------------------ jobs */
static const uint64_t FAKE = 1ull << 20; /* aligned, non-null, never touched */
static const uint64_t FAR = 1ull << 40;  /* between the buffers of a job */

enum Layout { L_FAST, L_MISALIGNED, L_SHORT_STRIDE, L_OPEN_SHORT_STRIDE, N_LAYOUTS };
static const char *const LAYOUT_NAME[] = {"fast", "misaligned", "stride<roundup64", "stride<len+16"};

/* a sound job of n records of 1400 bytes; buffer b keeps jobs of a duplex apart */
static NoiseAeadUniform uniform_job(uint32_t n, uint32_t lanes, Layout l, uint32_t rps, uint32_t flags, int b = 0)
{
    NoiseAeadUniform j = {};
    const uint64_t base = FAKE + (uint64_t)(4 * b + 1) * FAR;
    j.ctx = (const void *)FAKE;
    j.nonce_base = (const uint64_t *)FAKE;
    j.in = (const uint8_t *)(base + (l == L_MISALIGNED ? 8 : 0));
    j.out = (uint8_t *)(base + FAR);
    j.status = (uint8_t *)(base + 2 * FAR);
    j.in_stride = l == L_SHORT_STRIDE ? 1392 : (l == L_OPEN_SHORT_STRIDE ? 1408 : 1424);
    j.out_stride = 1424;
    j.recs_per_state = rps;
    j.n_records = n;
    j.len = 1400;
    j.lanes_per_record = lanes;
    j.flags = flags;
    return j;
}

static NoiseAeadRagged ragged_job(uint32_t n, uint32_t lanes, uint32_t flags)
{
    NoiseAeadRagged j = {};
    j.recs = (const NoiseAeadRecord *)FAKE;
    j.in = (const uint8_t *)(FAKE + FAR);
    j.out = (uint8_t *)(FAKE + 2 * FAR);
    j.n_records = n;
    j.lanes_per_record = lanes;
    j.flags = flags;
    return j;
}

static const uint32_t OPEN_FLAGS[] = {0, NOISE_AEAD_FLAG_ONE_PASS, NOISE_AEAD_FLAG_VERIFY_FIRST,
                                      NOISE_AEAD_FLAG_ONE_PASS | NOISE_AEAD_FLAG_VERIFY_FIRST, NOISE_AEAD_FLAG_CT_GHASH};
static const uint32_t ALL_LANES[] = {0, 1, 2, 3, 4, 5, 8, 16, 32, 64};
static const uint32_t ALL_RPS[] = {1, 13, 16, 32, 64, 256};

static std::vector<uint32_t> record_counts(uint32_t cus)
{
    std::vector<uint32_t> v = {0, 1, 63, 64, 512, 513, 16383, 16384, 65535, 65536, 131071, 131072,
                               1u << 20, (1u << 26) - 1, 1u << 26};
    if (cus) v.insert(v.end(), {512 * cus - 1, 512 * cus, 512 * cus + 1});
    return v;
}

/* ----------------------------------------------------------------- table */
static int g_lines;
static uint32_t g_cus_now;

/* the lane counts no kernel is built for are refused whatever the size: three sizes show it */
static bool skip(uint32_t n, uint32_t lanes) { return (lanes == 3 || lanes == 5) && n != 0 && n != 64 && n != 65536; }

static void line_end(int rc)
{
    printf(" => 0x%x\n", rc);
    ++g_lines;
}

static void t_uniform(int cipher, bool open, uint32_t n, uint32_t lanes, Layout l, uint32_t rps, uint32_t flags)
{
    const NoiseAeadUniform j = uniform_job(n, lanes, l, rps, flags);
    printf("U %s %s cus=%u n=%u k=%u %s rps=%u f=%u :", cipher == CHACHA ? "chacha" : "aes", open ? "open" : "seal",
           g_cus_now, n, lanes, LAYOUT_NAME[l], rps, flags);
    line_end(backend_uniform(cipher, &j, open));
}

struct Side { uint32_t n, lanes; Layout l; uint32_t rps, flags; };

static void t_duplex(int cipher, Side s, Side o)
{
    const NoiseAeadUniform sj = uniform_job(s.n, s.lanes, s.l, s.rps, s.flags, 0);
    const NoiseAeadUniform oj = uniform_job(o.n, o.lanes, o.l, o.rps, o.flags, 1);
    printf("D %s cus=%u n=%u/%u k=%u/%u %s/%s rps=%u/%u f=%u/%u :", cipher == CHACHA ? "chacha" : "aes", g_cus_now, s.n,
           o.n, s.lanes, o.lanes, LAYOUT_NAME[s.l], LAYOUT_NAME[o.l], s.rps, o.rps, s.flags, o.flags);
    line_end(backend_duplex(cipher, &sj, &oj));
}

static void t_ragged(int cipher, bool open, uint32_t n, uint32_t lanes, uint32_t flags)
{
    const NoiseAeadRagged j = ragged_job(n, lanes, flags);
    printf("R %s %s cus=%u n=%u k=%u f=%u :", cipher == CHACHA ? "chacha" : "aes", open ? "open" : "seal", g_cus_now, n,
           lanes, flags);
    line_end(backend_ragged(cipher, &j, open));
}

static void t_lanes(uint32_t n)
{
    printf("L n=%u : default %d/%d duplex %d/%d host_aes %d host_chacha", n, backend_lanes(0, CHACHA, n, 0),
           backend_lanes(0, AES, n, 0), backend_lanes(1, CHACHA, n, 0), backend_lanes(1, AES, n, 0),
           backend_lanes(3, AES, n, 0));
    for (uint32_t max_len : {0u, 64u, 200u, 1400u, 65519u}) printf(" %d", backend_lanes(2, CHACHA, n, max_len));
    printf("\n");
    ++g_lines;
}

/* every axis of the issue against the defaults of the others, on a device
   of `cus` CUs; full: all values, else the few each switch can move */
static void table_device(uint32_t cus, bool full)
{
    const bool wide = full && cus == 256; /* the axes no CU count touches run once */
    g_cus_now = cus;
    backend_device(cus, 2 * cus);
    const std::vector<uint32_t> counts = full ? record_counts(cus) : std::vector<uint32_t>{512, 65536, 131072};
    const std::vector<uint32_t> lanes = wide ? std::vector<uint32_t>(ALL_LANES, ALL_LANES + 10)
                                             : (full ? std::vector<uint32_t>{0, 1} : std::vector<uint32_t>{0, 4});
    const uint32_t F = NOISE_AEAD_FLAG_FAST;
    for (int cipher : {CHACHA, AES}) {
        if (cipher == AES && full && !wide) continue; /* the AES-GCM plans ask nothing of the device */
        for (int open = 0; open < 2; ++open) {
            for (uint32_t n : counts)
                for (uint32_t k : lanes)
                    if (!skip(n, k)) t_uniform(cipher, open, n, k, L_FAST, 256, 0);
            for (uint32_t n : counts)
                for (uint32_t k : lanes)
                    if (!skip(n, k)) t_ragged(cipher, open, n, k, F);
            for (uint32_t n : counts)
                for (uint32_t k : {0u, 4u}) t_ragged(cipher, open, n, k, 0);
            if (!wide) continue;
            for (uint32_t n : {64u, 65536u, 131072u})
                for (uint32_t k : {0u, 1u, 2u, 4u, 8u, 16u})
                    for (int l = 1; l < N_LAYOUTS; ++l) t_uniform(cipher, open, n, k, (Layout)l, 256, 0);
            for (uint32_t n : {512u, 65536u, 131072u})
                for (uint32_t k : {0u, 1u, 2u, 4u, 16u})
                    for (uint32_t rps : ALL_RPS) t_uniform(cipher, open, n, k, L_FAST, rps, 0);
            for (uint32_t n : {512u, 131072u})
                for (uint32_t k : {0u, 1u, 4u})
                    for (uint32_t f : OPEN_FLAGS) {
                        t_uniform(cipher, open, n, k, L_FAST, 256, f);
                        t_uniform(cipher, open, n, k, L_MISALIGNED, 256, f);
                        t_ragged(cipher, open, n, k, f | F);
                        t_ragged(cipher, open, n, k, f);
                    }
        }
        for (uint32_t n : counts)
            for (uint32_t k : lanes)
                if (k < 32 && !skip(n, k)) t_duplex(cipher, {n, k, L_FAST, 256, 0}, {n, k, L_FAST, 256, 0});
        if (!wide) continue;
        const uint32_t n = 65536;
        const uint32_t mixed_n[][2] = {{n, 512}, {131072, n}, {0, n}, {n, 0}, {1, 1u << 20}, {n - 1, n}};
        for (auto &m : mixed_n) t_duplex(cipher, {m[0], 0, L_FAST, 256, 0}, {m[1], 0, L_FAST, 256, 0});
        const uint32_t mixed_k[][2] = {{4, 8}, {1, 4}, {0, 1}, {1, 0}, {0, 4}, {4, 0}, {0, 8}, {2, 2}};
        for (auto &m : mixed_k) t_duplex(cipher, {n, m[0], L_FAST, 256, 0}, {n, m[1], L_FAST, 256, 0});
        for (int ls = 0; ls < N_LAYOUTS; ++ls)
            for (int lo = 0; lo < N_LAYOUTS; ++lo)
                for (uint32_t k : {0u, 4u}) t_duplex(cipher, {n, k, (Layout)ls, 256, 0}, {n, k, (Layout)lo, 256, 0});
        for (uint32_t k : {0u, 1u, 4u, 8u}) {
            for (uint32_t rps : ALL_RPS) {
                t_duplex(cipher, {n, k, L_FAST, rps, 0}, {n, k, L_FAST, 256, 0});
                t_duplex(cipher, {n, k, L_FAST, 256, 0}, {n, k, L_FAST, rps, 0});
                t_duplex(cipher, {n, k, L_FAST, rps, 0}, {n, k, L_FAST, rps, 0});
            }
            for (uint32_t fo : OPEN_FLAGS)
                for (uint32_t fs : {0u, (uint32_t)NOISE_AEAD_FLAG_CT_GHASH})
                    for (uint32_t m : {512u, n}) t_duplex(cipher, {m, k, L_FAST, 256, fs}, {m, k, L_FAST, 256, fo});
        }
    }
}

static void table_group(int g)
{
    backend_group(GROUPS[g]);
    printf("# %s=%s\n", GROUPS[g].name ? GROUPS[g].name : "defaults", GROUPS[g].name ? GROUPS[g].value : "");
    ++g_lines;
    for (uint32_t n : record_counts(0)) t_lanes(n);
    table_device(256, g == 0);
    if (g == 0) table_device(0, true), table_device(64, true);
}

/* ---------------------------------------------------------------- checks */
static int g_cases, g_fail;
#define CHECK(cond, ...)                                              \
    do {                                                              \
        ++g_cases;                                                    \
        if (!(cond) && ++g_fail <= 20) {                              \
            printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond);     \
            printf(__VA_ARGS__);                                      \
            printf("\n");                                             \
        }                                                             \
    } while (0)

enum { OK = NOISE_ERROR_NONE, PARAM = NOISE_ERROR_INVALID_PARAM, LENGTH = NOISE_ERROR_INVALID_LENGTH };

/* tests/test_abi.py test_device_api_argument_rules */
static void check_argument_rules()
{
    NoiseAeadUniform ok = {};
    ok.ctx = (const void *)FAKE, ok.nonce_base = (const uint64_t *)FAKE, ok.in = (const uint8_t *)FAKE;
    ok.out = (uint8_t *)(FAKE + (1ull << 30));
    ok.in_stride = 1408, ok.out_stride = 1424, ok.len = 1400, ok.n_records = 4, ok.recs_per_state = 4;
    NoiseAeadRagged rg = {};
    rg.recs = (const NoiseAeadRecord *)FAKE, rg.in = (const uint8_t *)FAKE, rg.out = (uint8_t *)FAKE, rg.n_records = 4;
    for (int open = 0; open < 2; ++open) {
        auto uni = [&](int cipher, NoiseAeadUniform j) { return backend_uniform(cipher, &j, open); };
        auto rag = [&](int cipher, NoiseAeadRagged j) { return backend_ragged(cipher, &j, open); };
        auto with = [](NoiseAeadUniform j, auto set) { set(j); return j; };
        for (int c : {CHACHA, AES}) {
            CHECK(uni(c, ok) == OK, "the sound job, cipher %x", c);
            CHECK(uni(c, with(ok, [](auto &j) { j.nonce_base = nullptr; })) == PARAM, "no nonces");
            CHECK(uni(c, with(ok, [](auto &j) { j.recs_per_state = 0; })) == PARAM, "rps 0");
            CHECK(uni(c, with(ok, [](auto &j) { j.ctx = (const void *)(FAKE + 8); })) == PARAM, "ctx alignment");
            CHECK(uni(c, with(ok, [](auto &j) { j.ad_len = 32; })) == PARAM, "AD length without AD");
            CHECK(uni(c, with(ok, [](auto &j) { j.len = 65520; })) == LENGTH, "length");
            CHECK(rag(c, [&] { auto j = rg; j.recs = nullptr; return j; }()) == PARAM, "no descriptors");
            CHECK(rag(c, [&] { auto j = rg; j.out = nullptr; return j; }()) == PARAM, "no output");
            CHECK(rag(c, rg) == OK, "the sound ragged job");
            /* records must be exactly in place or disjoint */
            CHECK(uni(c, with(ok, [](auto &j) { j.out = (uint8_t *)FAKE; })) == PARAM, "in == out, two strides");
            CHECK(uni(c, with(ok, [](auto &j) { j.out = (uint8_t *)(FAKE + 64), j.out_stride = 1408; })) == PARAM,
                  "output shifted into the input");
            CHECK(uni(c, with(ok, [](auto &j) { j.out = (uint8_t *)(FAKE + 4 * 1408 - 16); })) == PARAM, "spans touch");
            /* one stride, input and output slots alternating.  The
               accepted ones are checked here alone: through the library an
               accepted job is launched, which invented pointers must never be */
            const NoiseAeadUniform inter = with(ok, [](auto &j) { j.in_stride = j.out_stride = 2848; });
            CHECK(uni(c, with(inter, [](auto &j) { j.out = (uint8_t *)(FAKE + 1424); })) == OK, "interleaved above");
            CHECK(uni(c, with(inter, [](auto &j) { j.out = (uint8_t *)(FAKE - 1424); })) == OK, "interleaved below");
            CHECK(uni(c, with(inter, [](auto &j) { j.out = (uint8_t *)(FAKE + 1408); })) == (open ? PARAM : OK),
                  "the open's input holds the tag");
            CHECK(uni(c, with(inter, [](auto &j) { j.out = (uint8_t *)(FAKE + 1000); })) == PARAM, "records meet");
        }
        CHECK(uni(CHACHA, with(ok, [](auto &j) { j.lanes_per_record = 3; })) == PARAM, "3 lanes");
        CHECK(uni(CHACHA, with(ok, [](auto &j) { j.lanes_per_record = 128; })) == PARAM, "128 lanes");
        CHECK(uni(AES, with(ok, [](auto &j) { j.lanes_per_record = 8; })) == PARAM, "AES-GCM on 8 lanes");
        CHECK(uni(CHACHA, with(ok, [](auto &j) { j.n_records = 0; })) == OK, "empty job");
        CHECK(rag(CHACHA, [&] { auto j = rg; j.lanes_per_record = 5; return j; }()) == PARAM, "5 lanes");
        CHECK(rag(0x4399, rg) == NOISE_ERROR_UNKNOWN_ID, "unknown cipher");
        CHECK(uni(0x4399, ok) == NOISE_ERROR_UNKNOWN_ID, "unknown cipher");
    }
}

/* tests/test_abi.py test_duplex_independence_rules */
static void check_independence_rules()
{
    const uint64_t G = 1ull << 30;
    NoiseAeadUniform seal = {}, opn = {};
    seal.ctx = opn.ctx = (const void *)FAKE, seal.nonce_base = opn.nonce_base = (const uint64_t *)FAKE;
    seal.len = opn.len = 1400, seal.n_records = opn.n_records = 4, seal.recs_per_state = opn.recs_per_state = 4;
    seal.in = (const uint8_t *)(2 * G), seal.out = (uint8_t *)(3 * G), seal.in_stride = 1408, seal.out_stride = 1536;
    opn.in = (const uint8_t *)(4 * G), opn.out = (uint8_t *)(5 * G), opn.in_stride = 1536, opn.out_stride = 1408;
    opn.status = (uint8_t *)(6 * G);
    for (int c : {CHACHA, AES}) {
        auto duplex = [&](NoiseAeadUniform s, NoiseAeadUniform o) { return backend_duplex(c, &s, &o); };
        auto ad = [](NoiseAeadUniform j, uint64_t at, uint32_t len) {
            j.ad = (const uint8_t *)at, j.ad_len = len, j.ad_stride = len;
            return j;
        };
        NoiseAeadUniform o = opn;
        CHECK(duplex(seal, opn) == OK, "independent jobs");
        o.in = (const uint8_t *)(3 * G);
        CHECK(duplex(seal, o) == PARAM, "the open reads the seal's output");
        o = opn, o.out = (uint8_t *)(3 * G + 100);
        CHECK(duplex(seal, o) == PARAM, "outputs overlap");
        o = opn, o.out = (uint8_t *)(2 * G);
        CHECK(duplex(seal, o) == PARAM, "the open writes the seal's input");
        o = opn, o.status = (uint8_t *)(3 * G + 1536);
        CHECK(duplex(seal, o) == PARAM, "statuses in the seal's output");
        o = opn, o.status = (uint8_t *)(2 * G + 8);
        CHECK(duplex(seal, o) == PARAM, "statuses in the seal's input");
        CHECK(duplex(seal, ad(opn, 3 * G, 16)) == PARAM, "the open's AD in the seal's output");
        CHECK(duplex(ad(seal, 5 * G + 32, 8), opn) == PARAM, "the seal's AD in the open's output");
        CHECK(duplex(ad(seal, 6 * G, 8), opn) == PARAM, "the seal's AD in the open's statuses");
        CHECK(duplex(ad(seal, 7 * G, 8), ad(opn, 7 * G, 8)) == OK, "shared AD is only read");
    }
}

/* do any input and output record of the job meet (its records enumerated)?
   Exactly in place (the same slots) is no meeting. */
static bool brute_meet(const NoiseAeadUniform &j, bool open)
{
    if (j.in == j.out && j.in_stride == j.out_stride) return false;
    const u128 rin = j.len + (open ? 16u : 0u), rout = j.len + (open ? 0u : 16u);
    for (uint32_t i = 0; i < j.n_records; ++i)
        for (uint32_t k = 0; k < j.n_records; ++k) {
            const u128 a = (u128)(uintptr_t)j.in + (u128)i * j.in_stride, b = (u128)(uintptr_t)j.out + (u128)k * j.out_stride;
            if (rin && rout && a < b + rout && b < a + rin) return true;
        }
    return false;
}

/* Small jobs against the enumeration: with one stride that holds a record
   the check is exact; otherwise it asks for disjoint spans, which may refuse
   more than the records need but never less. */
static void check_against_enumeration()
{
    for (uint64_t base : {4096ull, (1ull << 63) - 64, (1ull << 63) + 4096})
        for (uint32_t n = 1; n <= 8; ++n)
            for (uint32_t len : {0u, 1u, 15u, 16u, 33u, 48u})
                for (int open = 0; open < 2; ++open)
                    for (uint64_t s_in : {1ull, len + 16ull, 2ull * len + 37, 128ull})
                        for (uint64_t s_out : {s_in, s_in + 16}) {
                            const int64_t reach = (int64_t)(n * (s_in > s_out ? s_in : s_out) + 80);
                            for (int64_t d = -reach; d <= reach; ++d) {
                                NoiseAeadUniform j = {};
                                j.ctx = (const void *)FAKE, j.nonce_base = (const uint64_t *)FAKE;
                                j.in = (const uint8_t *)base, j.out = (uint8_t *)(base + (uint64_t)d);
                                j.in_stride = s_in, j.out_stride = s_out, j.len = len, j.n_records = n;
                                j.recs_per_state = 1;
                                const bool refused = check_uniform(&j, open) == PARAM;
                                const bool met = brute_meet(j, open);
                                const bool exact = s_in == s_out && s_in >= (uint64_t)len + 16;
                                CHECK(exact ? refused == met : (refused || !met),
                                      "base %" PRIx64 " n %u len %u open %d strides %" PRIu64 "/%" PRIu64 " d %" PRId64
                                      ": refused %d, records meet %d",
                                      base, n, len, open, s_in, s_out, d, refused, met);
                            }
                        }
}

/* Pointers, strides and counts at the arithmetic edges: the answers that are
   plain, and no sanitizer report for any of them. */
static void check_arithmetic_edges()
{
    const uint64_t bases[] = {16, 4096, (1ull << 63) - 4096, 1ull << 63, (1ull << 63) + 4096, ~0ull - 65535};
    const uint64_t strides[] = {1, 1424, 1ull << 40};
    const uint32_t counts[] = {1, 2, 0xFFFFFFFFu};
    for (uint64_t in : bases)
        for (uint64_t out : bases)
            for (uint64_t s : strides)
                for (uint32_t n : counts)
                    for (int open = 0; open < 2; ++open) {
                        NoiseAeadUniform j = {};
                        j.ctx = (const void *)FAKE, j.nonce_base = (const uint64_t *)FAKE, j.status = (uint8_t *)in;
                        j.in = (const uint8_t *)in, j.out = (uint8_t *)out, j.in_stride = j.out_stride = s;
                        j.len = 1400, j.n_records = n, j.recs_per_state = 1;
                        j.ad = (const uint8_t *)out, j.ad_len = 7, j.ad_stride = s;
                        const int rc = check_uniform(&j, open);
                        if (in == out) CHECK(rc == OK, "exactly in place");
                        else if (n == 1) CHECK(rc == (meet(job_span(&j, false, open), job_span(&j, true, open)) ? PARAM : OK), "one record");
                        else CHECK(rc == OK || rc == PARAM, "rc %x", rc);
                        /* 2^32 - 1 records a stride of 2^40 apart reach every base above them:
                           they meet the output iff it lies within a record of a multiple of the stride */
                        if (n == 0xFFFFFFFFu && s == (1ull << 40) && in < out) {
                            const uint64_t r = (out - in) % s, rin = open ? 1416 : 1400, rout = open ? 1400 : 1416;
                            CHECK(rc == ((r < rin || s - r < rout) ? PARAM : OK),
                                  "interleaved at the widest: in %" PRIx64 " out %" PRIx64 " open %d rc %x", in, out, open, rc);
                        }
                        NoiseAeadUniform o = j;
                        o.in = (const uint8_t *)(out ^ (1ull << 62)), o.out = (uint8_t *)(in ^ (1ull << 62));
                        const int rd = check_duplex(&j, &o);
                        CHECK(rd == OK || rd == PARAM, "duplex rc %x", rd);
                        for (int c : {CHACHA, AES}) {
                            const Plan p = plan_uniform(c, &j, open, Switches(), 256);
                            CHECK(p.rc == OK && (p.grid > 0) == (n > 0), "plan at the edge: rc %x grid %u", p.rc, p.grid);
                            (void)plan_duplex(c, &j, &o, Switches(), 256);
                        }
                    }
}

/* ------------------------------------------------- the ragged duplex plan
   plan_duplex_ragged's promises, stated against plan_ragged (each job's
   plan alone): a shared launch runs, for each job, the family and template
   arguments the job would run alone. */
static int g_shared; /* shared plans seen */

static bool same_ragged_kernel(const Plan &a, const Plan &b)
{
    if (a.kernel != b.kernel) return false;
    switch (a.kernel) {
    case K_CHACHA_SEG_RAGGED: return true;
    case K_CHACHA_RAGGED: return a.lanes == b.lanes && a.fast == b.fast;
    case K_GCM_RAGGED: return a.wg == b.wg && a.r == b.r && a.lanes == b.lanes && a.fast == b.fast && a.ct == b.ct;
    default: return false; /* gcm_wide shares nothing */
    }
}

static void check_duplex_ragged_plan(int cipher, const NoiseAeadRagged &sj, const NoiseAeadRagged &oj, int sw_value,
                                     uint32_t resident)
{
    Switches sw;
    sw.ragged_duplex = sw_value;
    const Plan ps = plan_ragged(cipher, &sj, false, sw, resident), po = plan_ragged(cipher, &oj, true, sw, resident);
    const Plan p = plan_duplex_ragged(cipher, &sj, &oj, sw, resident);
#define WHERE "cipher %x n %u/%u k %u/%u f %u/%u sw %d resident %u", cipher, sj.n_records, oj.n_records, \
              sj.lanes_per_record, oj.lanes_per_record, sj.flags, oj.flags, sw_value, resident
    /* a refused standalone plan is refused here with the same rc */
    const int want_rc = ps.rc ? ps.rc : po.rc;
    CHECK(p.rc == want_rc, WHERE);
    if (want_rc) return;
    bool want = sw_value != 0 && sj.n_records && oj.n_records && same_ragged_kernel(ps, po);
    if (want && sw_value < 0) {
        Switches on;
        on.ragged_duplex = 1;
        const Plan forced = plan_duplex_ragged(cipher, &sj, &oj, on, resident);
        want = ragged_duplex_default(forced.kernel, forced.vf);
    }
    CHECK(p.shared == want, WHERE);
    g_shared += p.shared;
    if (!p.shared) {
        CHECK(p.kernel == K_NONE && !p.grid, WHERE);
        return;
    }
    /* shared implies: both standalone plans exist and name one family with
       the same template arguments */
    CHECK(!ps.rc && !po.rc && ps.grid && po.grid && same_ragged_kernel(ps, po), WHERE);
    CHECK(plan_is_gcm(p) == (cipher == AES), WHERE);
    CHECK(p.vf == po.vf && p.fast == ps.fast && p.fast == po.fast && p.park == p.grid, WHERE);
    char line[256];
    plan_print(p, line, sizeof line);
    CHECK(strstr(line, " sb=") && strstr(line, " ob="), "%s", line);
    switch (ps.kernel) {
    case K_CHACHA_SEG_RAGGED: {
        const uint64_t most = (uint64_t)blocks_for((uint64_t)sj.n_records * PLAN_SEG_KMAX, PLAN_BLOCK) +
                              blocks_for((uint64_t)oj.n_records * PLAN_SEG_KMAX, PLAN_BLOCK);
        CHECK(p.kernel == K_CHACHA_SEG_DUPLEX && p.grid == (most < resident ? most : resident) && p.block == PLAN_BLOCK, WHERE);
        CHECK(!strncmp(line, "chachapoly_seg_duplex ", 22), "%s", line);
        break;
    }
    case K_CHACHA_RAGGED:
        CHECK(p.kernel == K_CHACHA_DUPLEX_RAGGED && p.lanes == ps.lanes && p.vf_order == po.vf_order, WHERE);
        CHECK(p.sb == ps.grid && p.ob == po.grid && p.grid == p.sb + p.ob && p.block == PLAN_BLOCK, WHERE);
        CHECK(!strncmp(line, "chachapoly_duplex_ragged<", 25), "%s", line);
        break;
    case K_GCM_RAGGED:
        CHECK(p.kernel == K_GCM_DUPLEX_RAGGED && p.wg == ps.wg && p.r == ps.r && p.lanes == ps.lanes && p.ct == ps.ct, WHERE);
        CHECK(p.sb == ps.grid && p.ob == po.grid && p.grid == (p.sb > p.ob ? p.sb : p.ob) && p.block == ps.block, WHERE);
        CHECK(!strncmp(line, "gcm_duplex_ragged<", 18), "%s", line);
        break;
    default: CHECK(false, WHERE);
    }
#undef WHERE
}

static void check_duplex_ragged_plans()
{
    const uint32_t counts[] = {0, 1, 63, 64, 300, 512, 513, 16383, 16384, 65535, 65536, 131071, 131072, 1u << 26};
    const uint32_t lanes[] = {0, 1, 4, 8, 64};
    const uint32_t F = NOISE_AEAD_FLAG_FAST;
    const uint32_t flags[] = {0, F, F | NOISE_AEAD_FLAG_CT_GHASH, F | NOISE_AEAD_FLAG_ONE_PASS};
    for (int cipher : {CHACHA, AES})
        for (uint32_t ns : counts)
            for (uint32_t no : counts)
                for (uint32_t ks : lanes)
                    for (uint32_t ko : lanes)
                        for (uint32_t fs : flags)
                            for (uint32_t fo : flags)
                                for (int sw : {1, 0, -1})
                                    for (uint32_t resident : {0u, 512u})
                                        check_duplex_ragged_plan(cipher, ragged_job(ns, ks, fs), ragged_job(no, ko, fo), sw,
                                                                 resident);
    /* lanes no kernel is built for, and an unknown cipher */
    const NoiseAeadRagged ok = ragged_job(300, 8, F), bad = ragged_job(300, 3, F);
    Switches on;
    on.ragged_duplex = 1;
    CHECK(plan_duplex_ragged(CHACHA, &bad, &ok, on, 512).rc == PARAM, "3 lanes on the seal job");
    CHECK(plan_duplex_ragged(CHACHA, &ok, &bad, on, 512).rc == PARAM, "3 lanes on the open job");
    CHECK(plan_duplex_ragged(0x4303, &ok, &ok, on, 512).rc == NOISE_ERROR_UNKNOWN_ID, "unknown cipher");
}

/* check_duplex_ragged: the jobs' own checks, then the two status arrays */
static void check_duplex_ragged_spans()
{
    const NoiseAeadRagged ok = ragged_job(300, 0, 0);
    auto with = [&](uint64_t status, uint32_t n) {
        NoiseAeadRagged j = ok;
        j.status = (uint8_t *)status, j.n_records = n;
        return j;
    };
    auto rc = [](NoiseAeadRagged s, NoiseAeadRagged o) { return check_duplex_ragged(&s, &o); };
    CHECK(check_duplex_ragged(nullptr, &ok) == PARAM && check_duplex_ragged(&ok, nullptr) == PARAM, "a NULL job");
    for (int side = 0; side < 2; ++side) {
        NoiseAeadRagged j = ok;
        j.recs = nullptr;
        CHECK((side ? rc(ok, j) : rc(j, ok)) == PARAM, "no descriptors, side %d", side);
        j = ok, j.in = nullptr;
        CHECK((side ? rc(ok, j) : rc(j, ok)) == PARAM, "no input, side %d", side);
        j = ok, j.out = nullptr;
        CHECK((side ? rc(ok, j) : rc(j, ok)) == PARAM, "no output, side %d", side);
    }
    CHECK(rc(ok, ok) == OK, "no status arrays");
    for (uint64_t base : {4096ull, (1ull << 32) - 150, (1ull << 63) - 150, ~0ull - 1000}) {
        for (uint32_t n : {1u, 2u, 300u}) {
            CHECK(rc(with(base, n), with(base + n, n)) == OK, "arrays that touch: base %" PRIx64 " n %u", base, n);
            CHECK(rc(with(base + n, n), with(base, n)) == OK, "arrays that touch, swapped: base %" PRIx64 " n %u", base, n);
            CHECK(rc(with(base, n), with(base + n - 1, n)) == PARAM, "arrays that meet by a byte: base %" PRIx64 " n %u", base, n);
            CHECK(rc(with(base + n - 1, n), with(base, n)) == PARAM, "meet by a byte, swapped: base %" PRIx64 " n %u", base, n);
            CHECK(rc(with(base, n), with(base, n)) == PARAM, "one array for both: base %" PRIx64 " n %u", base, n);
            CHECK(rc(with(base, n), with(0, n)) == OK && rc(with(0, n), with(base, n)) == OK, "one array only");
            CHECK(rc(with(base, 0), with(base, n)) == OK && rc(with(base, n), with(base, 0)) == OK, "an empty job writes no status");
        }
    }
    /* the widest arrays: 2^32 - 1 statuses ending at the top of the address
       space (the span's end, 2^64 - 1, does not wrap in 128 bits) */
    const uint32_t N = 0xFFFFFFFFu;
    const uint64_t top = ~0ull - N;
    CHECK(rc(with(top, N), with(top - N, N)) == OK, "touch below the top");
    CHECK(rc(with(top, N), with(top - N + 1, N)) == PARAM, "meet by a byte below the top");
    CHECK(rc(with(top, N), with(16, N)) == OK, "a wrapped end would meet the bottom");
    CHECK(rc(with(~0ull, 1), with(16, 300)) == OK && rc(with(~0ull, 1), with(~0ull, 1)) == PARAM, "the last byte");
}

int main(int argc, char **argv)
{
    if (argc > 1 && !strcmp(argv[1], "--duplex-ragged")) {
        check_duplex_ragged_plans();
        check_duplex_ragged_spans();
        printf("dispatch_check: %d cases, %d failures, %d shared plans\n", g_cases, g_fail, g_shared);
        return g_fail ? 1 : 0;
    }
    if (argc > 1 && !strcmp(argv[1], "--groups")) {
        for (const EnvGroup &g : GROUPS) printf("%s=%s\n", g.name ? g.name : "", g.name ? g.value : "");
        return 0;
    }
    if (argc > 1 && !strcmp(argv[1], "--table")) {
        for (int g = 0; g < N_GROUPS; ++g)
            if (argc < 3 || atoi(argv[2]) == g) table_group(g);
        fprintf(stderr, "dispatch_check: %d table lines\n", g_lines);
        return 0;
    }
    g_quiet = true;
    backend_group(GROUPS[0]);
    backend_device(256, 512);
    check_argument_rules();
    check_independence_rules();
    check_arithmetic_edges();
    check_against_enumeration();
    printf("dispatch_check: %d cases, %d failures\n", g_cases, g_fail);
    return g_fail ? 1 : 0;
}
