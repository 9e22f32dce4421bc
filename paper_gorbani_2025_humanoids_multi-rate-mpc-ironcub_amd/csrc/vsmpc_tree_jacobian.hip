// Forward-mode Jacobian of what the kinematic-tree plant of the rollout hands a tick (vsmpc_tree_jacobian_batch):
//   (q[8], T[4]) -> tau = A_mom,body 6x4 | Lambda_lin,B 3x8 | Lambda_ang,B 3x8 | I_B 3x3     (VSMPC_TT_*, 81 numbers)
// and J = d tau / d(q | T), 81 x 12, at the pose tree_state_kernel gives the provider in a rollout: base at the origin,
// identity attitude, at rest.  The arithmetic is provider_kernel's and kinematics_kernel's for that pose (R_base = 1 and
// p_base = 0 drop out; I_B = [S(r); 1]^T M_b [S(r); 1] with r = CoM is I_O + m S(r)^2), carried as value-and-derivative pairs.
//
// Lanes: 16 per instance, 4 instances per wavefront.  Lane j < 8 of a group carries the direction d/dq_j through the whole
// chain and writes column j of J and (lane 0) tau.  Lambda is linear in T, so the thrust columns need no direction of their
// own: column 8 + i is Lambda's jet-i summand before it is scaled, which lane i of the group writes on its way.  Lanes 8..15
// of a group idle.  No lane reads what another lane's direction produced: no reduction, no barrier, no atomics.
//
// The provider walks its bodies by the run-time parent[] / jet_body[] tables, so the per-body frames cannot live in registers
// (a dynamically indexed private array is scratch memory).  They are staged in LDS: the values once per group (all eight
// lanes store the same number), the derivatives per lane, lane-minor so that a wavefront's access is conflict-free.
#include "vsmpc_device.hpp"
#include "vsmpc_launch.hpp"

namespace vsmpc {

namespace {

constexpr int NB = VSMPC_TREE_NB, NJT = VSMPC_TREE_NJ, NJETS = VSMPC_N_THRUSTS;
constexpr int TJ_GROUPS = 4, TJ_LANES = 16, TJ_DIRS = 8;     // instances per block, lanes per instance, of them with a direction
// LDS slots of one instance (triples unless said otherwise)
constexpr int SL_R = 0;                     // 9 x 9 body frames
constexpr int SL_P = SL_R + 9 * NB;         // body origins; joint j's origin is P[j + 1]
constexpr int SL_AX = SL_P + 3 * NB;        // joint axes
constexpr int SL_C = SL_AX + 3 * NJT;       // body CoMs
constexpr int SL_JET = SL_C + 3 * NB;       // per jet: position | axis
constexpr int SL_SIZE = SL_JET + 6 * NJETS;

struct D {   // value and derivative along the lane's direction
    double v, d;
};
__host__ __device__ __forceinline__ D operator+(D a, D b) { return {a.v + b.v, a.d + b.d}; }
__host__ __device__ __forceinline__ D operator-(D a, D b) { return {a.v - b.v, a.d - b.d}; }
__host__ __device__ __forceinline__ D operator*(D a, D b) { return {a.v * b.v, a.d * b.v + a.v * b.d}; }
__host__ __device__ __forceinline__ D operator*(double a, D b) { return {a * b.v, a * b.d}; }
__host__ __device__ __forceinline__ D dconst(double a) { return {a, 0.0}; }

struct Stage {   // one lane's view of the staged frames: shared values, own derivatives
    double* val;
    double* der;
    __host__ __device__ __forceinline__ D get(int i) const { return {val[i], der[i * (TJ_GROUPS * TJ_DIRS)]}; }
    __host__ __device__ __forceinline__ void put(int i, D x) const { val[i] = x.v; der[i * (TJ_GROUPS * TJ_DIRS)] = x.d; }
    __host__ __device__ __forceinline__ void get3(int i, D* o) const { o[0] = get(i); o[1] = get(i + 1); o[2] = get(i + 2); }
    __host__ __device__ __forceinline__ void put3(int i, const D* x) const { put(i, x[0]); put(i + 1, x[1]); put(i + 2, x[2]); }
};

__host__ __device__ __forceinline__ void cross3(const D* a, const D* b, D* o) {
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}
// R v with R the staged frame at slot `r` and v a constant of the tree
__host__ __device__ __forceinline__ void rot_const(const Stage& s, int r, const double* v, D* o) {
    for (int i = 0; i < 3; ++i) o[i] = v[0] * s.get(r + 3 * i) + v[1] * s.get(r + 3 * i + 1) + v[2] * s.get(r + 3 * i + 2);
}
__host__ __device__ __forceinline__ void unit3(const double* a, double* o) {
    const double nrm = 1.0 / sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
    for (int i = 0; i < 3; ++i) o[i] = a[i] * nrm;
}
// the tree joint behind robot joint `col` (the last one, as the provider's column writes leave it), or -1
__host__ __device__ __forceinline__ int joint_of_column(const vsmpc_tree& tree, int col) {
    int j = -1;
    for (int k = 0; k < NJT; ++k) j = tree.robot_joint[k] == col ? k : j;
    return j;
}

// One lane's work: direction d/dq_l (l < 8) through the whole chain for one instance; `s` and `anc` are the lane's staging.
// (A host compiler may run it too, lane after lane: no lane depends on another.)
__host__ __device__ __forceinline__ void tree_jacobian_lane(const vsmpc_tree& tree, const KinOpts& opts, const double* qb, const double* Tb,
                                                            int l, const Stage& s, int* anc, double* to, double* jo) {
    // one of the 81: its value (lane 0), its derivative along the lane's joint, and a zero thrust column from lanes 0..3
    auto emit = [&](int e, D x) {
        if (to != nullptr) to[e] = x.v;
        if (jo != nullptr) {
            jo[e * VSMPC_TT_NDIR + l] = x.d;
            if (l < NJETS) jo[e * VSMPC_TT_NDIR + TJ_DIRS + l] = 0.0;
        }
    };
    // ---- forward kinematics: bodies in index order (parents precede children)
    for (int i = 0; i < 9; ++i) s.put(SL_R + i, dconst(i % 4 == 0 ? 1.0 : 0.0));
    for (int i = 0; i < 3; ++i) s.put(SL_P + i, dconst(0.0));
    anc[0] = 0;
    for (int j = 0; j < NJT; ++j) {
        const int b = j + 1, par = tree.parent[b], rp = SL_R + 9 * par;
        double ax[3];
        unit3(&tree.joint_axis[3 * j], ax);
        D o[3], pp[3], aw[3];
        rot_const(s, rp, &tree.joint_origin[3 * j], o);
        s.get3(SL_P + 3 * par, pp);
        for (int i = 0; i < 3; ++i) s.put(SL_P + 3 * b + i, pp[i] + o[i]);
        rot_const(s, rp, ax, aw);
        s.put3(SL_AX + 3 * j, aw);
        // Rodrigues: Rj = I + sin K + (1 - cos) K^2; the lane's direction enters at its own joint
        double sn, cs;
        sincos(qb[j], &sn, &cs);
        const double seed = l == j ? 1.0 : 0.0;
        const D dsn{sn, cs * seed}, dvc{1.0 - cs, sn * seed};
        const double Kx[9] = {0.0, -ax[2], ax[1], ax[2], 0.0, -ax[0], -ax[1], ax[0], 0.0};
        D Rj[9];
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) {
                double k2 = 0.0;
                for (int t = 0; t < 3; ++t) k2 += Kx[3 * r + t] * Kx[3 * t + c];
                Rj[3 * r + c] = dconst(r == c ? 1.0 : 0.0) + Kx[3 * r + c] * dsn + k2 * dvc;
            }
        for (int r = 0; r < 3; ++r) {
            D row[3];
            s.get3(rp + 3 * r, row);
            for (int c = 0; c < 3; ++c) s.put(SL_R + 9 * b + 3 * r + c, row[0] * Rj[c] + row[1] * Rj[3 + c] + row[2] * Rj[6 + c]);
        }
        anc[b] = anc[par] | (1 << j);
    }
    // ---- bodies: CoMs, total mass, CoM, inertia about the base origin
    double m = 0.0;
    D com[3] = {dconst(0.0), dconst(0.0), dconst(0.0)}, IO[9];
    for (int i = 0; i < 9; ++i) IO[i] = dconst(0.0);
    for (int b = 0; b < NB; ++b) {
        D c[3], pb[3];
        rot_const(s, SL_R + 9 * b, &tree.com[3 * b], c);
        s.get3(SL_P + 3 * b, pb);
        for (int i = 0; i < 3; ++i) c[i] = pb[i] + c[i];
        s.put3(SL_C + 3 * b, c);
        const double mb = tree.mass[b];
        m += mb;
        for (int i = 0; i < 3; ++i) com[i] = com[i] + mb * c[i];
        const double* in = &tree.inertia[6 * b];
        const double Ib[9] = {in[0], in[1], in[2], in[1], in[3], in[4], in[2], in[4], in[5]};
        D RI[9];     // R I_b, then (R I_b) R^T
        for (int r = 0; r < 3; ++r) {
            D row[3];
            s.get3(SL_R + 9 * b + 3 * r, row);
            for (int cc = 0; cc < 3; ++cc) RI[3 * r + cc] = Ib[cc] * row[0] + Ib[3 + cc] * row[1] + Ib[6 + cc] * row[2];
        }
        const D dd = c[0] * c[0] + c[1] * c[1] + c[2] * c[2];
        for (int cc = 0; cc < 3; ++cc) {
            D row[3];
            s.get3(SL_R + 9 * b + 3 * cc, row);
            for (int r = 0; r < 3; ++r) {
                D v = RI[3 * r] * row[0] + RI[3 * r + 1] * row[1] + RI[3 * r + 2] * row[2];
                if (r == cc) v = v + mb * dd;
                IO[3 * r + cc] = IO[3 * r + cc] + v - mb * (c[r] * c[cc]);
            }
        }
    }
    for (int i = 0; i < 3; ++i) com[i] = (1.0 / m) * com[i];
    {   // I_B = I_O - m (|c|^2 1 - c c^T)
        const D cc2 = com[0] * com[0] + com[1] * com[1] + com[2] * com[2];
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) {
                D v = IO[3 * r + c] + m * (com[r] * com[c]);
                if (r == c) v = v - m * cc2;
                emit(VSMPC_TT_IB + 3 * r + c, v);
            }
    }
    // ---- jets: position, axis; A_mom,body = [a_i; r_i x a_i], r_i = p_i - CoM
    for (int i = 0; i < NJETS; ++i) {
        const int b = tree.jet_body[i];
        double al[3];
        unit3(&tree.jet_axis[3 * i], al);
        D o[3], a[3], pb[3], r[3], ra[3];
        rot_const(s, SL_R + 9 * b, &tree.jet_origin[3 * i], o);
        rot_const(s, SL_R + 9 * b, al, a);
        s.get3(SL_P + 3 * b, pb);
        for (int t = 0; t < 3; ++t) { o[t] = pb[t] + o[t]; r[t] = o[t] - com[t]; }
        s.put3(SL_JET + 6 * i, o);
        s.put3(SL_JET + 6 * i + 3, a);
        cross3(r, a, ra);
        for (int t = 0; t < 3; ++t) {
            emit(VSMPC_TT_AMOM + 4 * t + i, a[t]);
            emit(VSMPC_TT_AMOM + 4 * (3 + t) + i, ra[t]);
        }
    }
    // ---- Lambda, column by column: linear columns are robot joints 3..10 (systemDynamicsVSMPC.cpp:348), angular ones the
    // handle's selector; per jet  lin = -T a x Jrel,  ang = -T (a x (Jframe - Jcom) + r x (a x Jrel))
    for (int pass = 0; pass < 2; ++pass)
        for (int c = 0; c < VSMPC_N_JOINTS; ++c) {
            const bool ang = pass == 1;
            const int j = joint_of_column(tree, ang ? opts.sel[c] : 3 + c);
            const int base = (ang ? VSMPC_TT_LANG : VSMPC_TT_LLIN) + c;
            D axj[3], org[3], jc[3] = {dconst(0.0), dconst(0.0), dconst(0.0)}, sum[3] = {dconst(0.0), dconst(0.0), dconst(0.0)};
            if (j >= 0) {
                s.get3(SL_AX + 3 * j, axj);
                s.get3(SL_P + 3 * (j + 1), org);
                if (ang) {   // CoM Jacobian column
                    for (int b = 1; b < NB; ++b)
                        if (anc[b] & (1 << j)) {
                            D cb[3], d[3], x[3];
                            s.get3(SL_C + 3 * b, cb);
                            for (int t = 0; t < 3; ++t) d[t] = cb[t] - org[t];
                            cross3(axj, d, x);
                            for (int t = 0; t < 3; ++t) jc[t] = jc[t] + tree.mass[b] * x[t];
                        }
                    for (int t = 0; t < 3; ++t) jc[t] = (1.0 / m) * jc[t];
                }
            }
            for (int i = 0; i < NJETS; ++i) {
                D term[3] = {dconst(0.0), dconst(0.0), dconst(0.0)};
                if (j >= 0) {
                    const bool on = (anc[tree.jet_body[i]] >> j) & 1;
                    D pj[3], a[3], w[3] = {dconst(0.0), dconst(0.0), dconst(0.0)};
                    s.get3(SL_JET + 6 * i, pj);
                    s.get3(SL_JET + 6 * i + 3, a);
                    if (on) cross3(a, axj, w);                       // S(a) Jrel
                    if (!ang) {
                        for (int t = 0; t < 3; ++t) term[t] = dconst(0.0) - w[t];
                    } else {
                        D d[3], jf[3] = {dconst(0.0), dconst(0.0), dconst(0.0)}, u[3], r[3], z[3];
                        if (on) {
                            for (int t = 0; t < 3; ++t) d[t] = pj[t] - org[t];
                            cross3(axj, d, jf);
                        }
                        for (int t = 0; t < 3; ++t) { jf[t] = jf[t] - jc[t]; r[t] = pj[t] - com[t]; }
                        cross3(a, jf, u);
                        cross3(r, w, z);
                        for (int t = 0; t < 3; ++t) term[t] = dconst(0.0) - (u[t] + z[t]);
                    }
                }
                const double Ti = Tb[i];
                for (int t = 0; t < 3; ++t) {
                    sum[t] = sum[t] + Ti * term[t];
                    if (jo != nullptr && l == i) jo[(base + 8 * t) * VSMPC_TT_NDIR + TJ_DIRS + i] = term[t].v;
                }
            }
            for (int t = 0; t < 3; ++t) {
                if (to != nullptr) to[base + 8 * t] = sum[t].v;
                if (jo != nullptr) jo[(base + 8 * t) * VSMPC_TT_NDIR + l] = sum[t].d;
            }
        }
}

}  // namespace

__global__ __launch_bounds__(TJ_GROUPS* TJ_LANES) void tree_jacobian_kernel(vsmpc_tree tree, KinOpts opts,
                                                                            const double* __restrict__ q, int q_stride,
                                                                            const double* __restrict__ thrust, int t_stride, int batch,
                                                                            double* __restrict__ terms, double* __restrict__ jac) {
    __shared__ double sVal[TJ_GROUPS][SL_SIZE];
    __shared__ double sDer[SL_SIZE][TJ_GROUPS * TJ_DIRS];
    __shared__ int sAnc[TJ_GROUPS][NB];          // joints between the base and the body, as a bit mask
    const int g = threadIdx.x / TJ_LANES, l = threadIdx.x % TJ_LANES;
    const int b0 = blockIdx.x * TJ_GROUPS + g;
    if (b0 >= batch || l >= TJ_DIRS) return;     // (no barrier below)
    const Stage s{sVal[g], &sDer[0][g * TJ_DIRS + l]};
    tree_jacobian_lane(tree, opts, q + size_t(b0) * q_stride, thrust + size_t(b0) * t_stride, l, s, sAnc[g],
                       terms != nullptr && l == 0 ? terms + size_t(b0) * VSMPC_TT_SIZE : nullptr,
                       jac != nullptr ? jac + size_t(b0) * VSMPC_TT_SIZE * VSMPC_TT_NDIR : nullptr);
}

hipError_t launch_tree_jacobian(const vsmpc_tree& tree, const KinOpts& opts, const double* d_q, int q_stride, const double* d_thrust,
                                int t_stride, int batch, double* d_terms, double* d_jac, hipStream_t stream) {
    hipLaunchKernelGGL(tree_jacobian_kernel, dim3((batch + TJ_GROUPS - 1) / TJ_GROUPS), dim3(TJ_GROUPS * TJ_LANES), 0, stream, tree,
                       opts, d_q, q_stride, d_thrust, t_stride, batch, d_terms, d_jac);
    return hipGetLastError();
}

}  // namespace vsmpc
