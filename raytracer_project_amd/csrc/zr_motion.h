// zr_motion.h — the motion of a refit: every world-list entry's object-to-world affine map M, and for an entry a refit moved the record the temporal
// stage reprojects its pixels with: A = M_prev · M_now⁻¹ (a world point of the entry now -> where that point of the entry was one epoch ago) and the normal map
// Nm = (A_lin)⁻ᵀ.  FP64, one fixed operation order, compiled with -ffp-contract=off; no HIP in here, like zr_update.h: zr_update.cpp includes it for the library,
// tests/native/motion_check.cpp compiles it alone.
//   M     the entry's chain applied innermost first with put_triangle's forward point maps (zr_entry.h): translate p + a; rotate_x/y/z (co a - sn b, sn a + co b);
//         scale p a component-wise; material nothing.  A medium's inner chain sits inside the entry's own; an entry whose leaf primitive is a sphere
//         zr_scene_update_spheres can reach starts from the sphere's own map x -> c + max(0, r) x.
//   record   21 doubles: a[12] = per row k the linear part a[4k .. 4k+2] and the translation a[4k+3]; nm[9] by rows.  Every value has +0.0 added (no -0).
//   cut   the entry cannot be followed — a 3x3 determinant that is 0 or not finite (a radius or scale factor of 0 on either side), or a value of the record that
//         is not finite: its pixels get no history.
#pragma once
#include "zr_update.h"

namespace {

constexpr uint32_t kMotionStatic = ZR_MOTION_STATIC, kMotionCut = ZR_MOTION_CUT;
constexpr int kMotionDoubles = 21;

struct Affine {   // row k: m[4k .. 4k+2] linear, m[4k+3] translation
    double m[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    // op ∘ this
    void apply(const zr_xform_op& op) {
        if (op.kind == ZR_OP_TRANSLATE) { for (int k = 0; k < 3; k++) m[4 * k + 3] = m[4 * k + 3] + op.a[k]; }
        else if (op.kind == ZR_OP_SCALE) { for (int k = 0; k < 3; k++) for (int c = 0; c < 4; c++) m[4 * k + c] = m[4 * k + c] * op.a[k]; }
        else if (op.kind == ZR_OP_ROTATE_X || op.kind == ZR_OP_ROTATE_Y || op.kind == ZR_OP_ROTATE_Z) {
            const double sn = op.a[0], co = op.a[1];
            const int ra = op.kind == ZR_OP_ROTATE_X ? 1 : 0, rb = op.kind == ZR_OP_ROTATE_Z ? 1 : 2;   // the (a, b) plane of zr_entry.h's rotations
            for (int c = 0; c < 4; c++) {
                const double a = m[4 * ra + c], b = m[4 * rb + c];
                m[4 * ra + c] = co * a - sn * b; m[4 * rb + c] = sn * a + co * b;
            }
        }
    }
    void apply_chain(const zr_xform_op* ops, uint32_t first, uint32_t count) { for (int k = (int)count - 1; k >= 0; k--) apply(ops[first + k]); }
};

// the map of world-list entry oi over the current host arrays (a leaf sphere of its own: UpdateIndex::build_reverse's leaf_sphere)
inline Affine entry_map(const UpdateWorld& w, uint32_t oi) {
    const zr_object& o = w.objs[oi];
    Affine M;
    if (o.type == ZR_PRIM_SPHERE && w.kind(oi) == ZR_PRIM_SPHERE) {
        const double* q = w.s.spheres.data() + (size_t)o.index * 4;
        const double r = std::fmax(0.0, q[3]);
        for (int k = 0; k < 3; k++) { M.m[4 * k + k] = r; M.m[4 * k + 3] = q[k]; }
    }
    if (o.type == ZR_PRIM_MEDIUM) { const zr_medium& md = w.s.media[o.index]; M.apply_chain(w.s.ops.data(), md.chain_first, md.chain_count); }
    M.apply_chain(w.s.ops.data(), o.chain_first, o.chain_count);
    return M;
}

// the inverse of the 3x3 in rows of stride `st`, by cofactors over the determinant, into rows of stride 3; false: det is 0 or not finite
inline bool inverse3(const double* l, int st, double* inv) {
    const double a = l[0], b = l[1], c = l[2], d = l[st], e = l[st + 1], f = l[st + 2], g = l[2 * st], h = l[2 * st + 1], i = l[2 * st + 2];
    const double c00 = e * i - f * h, c01 = f * g - d * i, c02 = d * h - e * g;
    const double det = (a * c00 + b * c01) + c * c02;
    if (!(std::isfinite(det) && det != 0.0)) return false;
    inv[0] = c00 / det; inv[1] = (c * h - b * i) / det; inv[2] = (b * f - c * e) / det;
    inv[3] = c01 / det; inv[4] = (a * i - c * g) / det; inv[5] = (c * d - a * f) / det;
    inv[6] = c02 / det; inv[7] = (b * g - a * h) / det; inv[8] = (a * e - b * d) / det;
    return true;
}

// rec[21] for an entry that went from `prev` to `now`; false: cut
inline bool motion_record(const Affine& prev, const Affine& now, double* rec) {
    double li[9], ti[3];   // M_now⁻¹ = (li, ti): li = L_now⁻¹, ti = -(li t_now)
    if (!inverse3(now.m, 4, li)) return false;
    for (int k = 0; k < 3; k++) ti[k] = 0.0 - ((li[3 * k] * now.m[3] + li[3 * k + 1] * now.m[7]) + li[3 * k + 2] * now.m[11]);
    double al[9];
    for (int k = 0; k < 3; k++) {
        const double* p = prev.m + 4 * k;
        for (int c = 0; c < 3; c++) al[3 * k + c] = (p[0] * li[c] + p[1] * li[3 + c]) + p[2] * li[6 + c];
        rec[4 * k + 3] = ((p[0] * ti[0] + p[1] * ti[1]) + p[2] * ti[2]) + p[3];
        for (int c = 0; c < 3; c++) rec[4 * k + c] = al[3 * k + c];
    }
    double ai[9];
    if (!inverse3(al, 3, ai)) return false;
    for (int k = 0; k < 3; k++) for (int c = 0; c < 3; c++) rec[12 + 3 * k + c] = ai[3 * c + k];   // the transpose of the inverse
    for (int k = 0; k < kMotionDoubles; k++) { rec[k] = rec[k] + 0.0; if (!std::isfinite(rec[k])) return false; }
    return true;
}

// The table of one refit on the host: the previous epoch's map of every movable entry, and what the last refit made of its dirty entries.
struct MotionTable {
    std::vector<uint32_t> map_of;    // per entry: its index among the movable ones, or kNoSlot
    std::vector<Affine> prev;        // per movable entry: M as of the previous epoch
    std::vector<uint32_t> entries;   // the entries the last refit touched, in its dirty order ...
    std::vector<uint32_t> slot;      // ... each one's slot among the records, or kMotionCut
    std::vector<double> records;     // 21 doubles per slot
    // before the first update changes anything: the maps of the committed world
    void build(const UpdateWorld& w) {
        const size_t n = w.objs.size();
        map_of.assign(n, kNoSlot); prev.clear();
        for (size_t oi = 0; oi < n; oi++) {
            bool reach = false;
            UpdateIndex::ops_of(w, (uint32_t)oi, [&](uint32_t) { reach = true; });
            if (w.objs[oi].type == ZR_PRIM_SPHERE && w.kind(oi) == ZR_PRIM_SPHERE) reach = true;
            if (reach) { map_of[oi] = (uint32_t)prev.size(); prev.push_back(entry_map(w, (uint32_t)oi)); }
        }
        clear();
    }
    void clear() { entries.clear(); slot.clear(); records.clear(); }
    // one refit: the dirty entries' records against their previous maps, which then advance
    void step(const UpdateWorld& w, const std::vector<uint32_t>& dirty_list) {
        clear();
        for (uint32_t oi : dirty_list) {
            const Affine now = entry_map(w, oi);
            Affine& was = prev[map_of[oi]];
            double rec[kMotionDoubles];
            entries.push_back(oi);
            if (motion_record(was, now, rec)) { slot.push_back((uint32_t)(records.size() / kMotionDoubles)); records.insert(records.end(), rec, rec + kMotionDoubles); }
            else slot.push_back(kMotionCut);
            was = now;
        }
    }
};

}  // namespace
