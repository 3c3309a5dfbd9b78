// hq_commit.hip — hq_commit_dev and hq_commit_many_dev, and the commit kernels over u64 columns
// (k_commit / k_commit_big with TILED = 0, bodies in hq_commit.h). A tiled batch goes on to
// hq_commit_tiles.hip, which holds the tile kernels, the fused launch and the tile packer.
//
// The column kernels are HBM streams over structure-of-arrays group state: one lane owns two
// groups (one where a column is not 16-byte aligned), consecutive lanes read consecutive groups,
// the decision is an integer min/max network in registers (hq_commit_body.h), and the changed /
// fallback bitmaps are assembled with wave-wide __ballot. No LDS and no MFMA: nothing is reused
// or a contraction (DESIGN.md "Kernels").
#include "hq_commit.h"

extern "C" int hq_commit_dev(hq_ctx *ctx, const hq_commit_args *a) {
    int rc = validate_commit(ctx, a);
    if (rc || a->G == 0) return rc;
    if (a->layout != HQ_LAYOUT_COLUMNS) return hq::launch_commit_tiles(ctx, a);
    const CommitK k = commit_k(a);
    const bool vec2 = commit_vec2(a);
    return dispatch_n(a->n_max, [&](auto n) {
        return dispatch<HQ_FORM_TERM_START, HQ_FORM_TERM_MASK, HQ_FORM_TERM_RING32,
                        HQ_FORM_TERM_RING>(a->form, [&](auto form) {
            return dispatch_bool(a->n_voting != nullptr, [&](auto pern) {
                return dispatch<2, 1>(vec2 ? 2 : 1, [&](auto vec) {
                    return launch_commit_t<decltype(n)::value, decltype(form)::value,
                                           decltype(vec)::value, decltype(pern)::value>(ctx, k);
                });
            });
        });
    });
}

extern "C" int hq_commit_many_dev(hq_ctx *ctx, const hq_commit_args *args, uint32_t count) {
    if (!ctx) return HQ_E_INVAL;
    if (count && !args) return hq::fail(ctx, HQ_E_INVAL, "hq_commit_many_dev: args is NULL");
    for (uint32_t i = 0; i < count; ++i) {
        int rc = hq_commit_dev(ctx, args + i);
        if (rc) return rc;
    }
    return HQ_OK;
}
