/*
 * ppenv_oracle.c — CPU restatement of the HumanoidPingpong VecTask step.
 *
 * TEST INFRASTRUCTURE ONLY.  Nothing under oracle/ is part of the product: only
 * tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may load it,
 * and only as the checker / reported CPU baseline.  The product path
 * (isaacgym_amd/) never links, imports or falls back to this file.
 *
 * What it restates, and from where (paths relative to /root/reference):
 *   - step order          tasks/humanoid_pingpong_3_actor_tilt.py:1002-1052 (TT)
 *   - action -> PD target  TT:1003-1014, limits -> offset/scale TT:649-671
 *   - reward / reset rule  TT:1105-1270 (TT), T3 = tasks/humanoid_interos_edit_pingpong_only_3_actor.py:1080-1173,
 *                          TN = tasks/humanoid_pingpong_3_actor_tilt_no_earlystop.py:1115-1322
 *   - masked reset         TT:847-906, T3:825-881, TN:871-917 (TN leaves dof state alone)
 *   - serve velocity       TT:296-323, T3:289-305, TN:301-328
 *   - observations         TT:1640-1708, with calc_heading_quat_inv / my_quat_rotate restated from the
 *                          published isaacgymenvs.utils.torch_jit_utils (un-vendored dependency, unpinned)
 *   - 4-actor variant      T4 = tasks/humanoid_pingpong_4_actor_tilt.py: rewards T4:1113-1439, reset T4:853-912, serve
 *                          T4:299-326, poses T4:525-526,555-556; the two-agent wiring the class leaves open (T4:743,786-803)
 *                          is the build's completion, stated in include/ppenv.h at PPENV_VARIANT_T4
 *
 * PARITY PINNING.  The reward / observation / reset part is pinned against the
 * reference's own torch functions: the npz files under tests/golden hold their outputs on
 * scripted state sequences (tools/gen_golden.py imports the reference in the
 * build container).  The rigid-body part (gym.simulate) is closed-source Isaac
 * Gym / PhysX, absent from the reference and from this pipeline, and no
 * reference test pins its results: for physics this oracle restates the
 * build's own written specification (DESIGN.md "Physics specification") —
 * PARITY UNPINNED for that part.  To make it a real check it deliberately uses
 * a different algorithm and precision from the HIP kernel: recursive
 * Newton-Euler in world coordinates + joint-space inertia matrix + dense
 * solve, in double precision (the kernel runs the articulated-body algorithm
 * in link coordinates in fp32).
 *
 * Reward, reset and observation arithmetic is fp32 in the reference's operation
 * order, so thresholds flip at the same inputs.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../include/ppenv.h"

#define ND PPENV_NUM_DOF
#define NB PPENV_NUM_OBS_BODIES

typedef struct ppo_env {
    ppenv_config cfg;
    int n;
    int A;   /* agents (humanoids) per env: 1, or 2 for PPENV_VARIANT_T4; agent a of env e owns row A*e + a of obs / rew / reset / progress */
    float *obs, *rew;
    int64_t *reset, *progress;
    float *dof_pos, *dof_vel, *dof_force, *ball; /* SoA [k][N] */
    uint32_t *flags, *episode;
    float *serve; /* [3][N] */
    int serve_on;
    ppenv_config* cfg_env;   /* domain randomisation: one scaled copy of cfg per env, or NULL */
    float dr_action_sigma, dr_obs_sigma;
    int threads;
} ppo_env;

/* ------------------------------------------------------------------ small math */
typedef struct { double x, y, z; } v3;
typedef struct { double m[9]; } m3;

static v3 V(double x, double y, double z) { v3 r = {x, y, z}; return r; }
static v3 vadd(v3 a, v3 b) { return V(a.x + b.x, a.y + b.y, a.z + b.z); }
static v3 vsub(v3 a, v3 b) { return V(a.x - b.x, a.y - b.y, a.z - b.z); }
static v3 vscale(v3 a, double s) { return V(a.x * s, a.y * s, a.z * s); }
static double vdot(v3 a, v3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
static v3 vcross(v3 a, v3 b) { return V(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }
static double vnorm(v3 a) { return sqrt(vdot(a, a)); }
static v3 vf(const float* p) { return V(p[0], p[1], p[2]); }
static v3 mv(const m3* a, v3 v) {
    return V(a->m[0] * v.x + a->m[1] * v.y + a->m[2] * v.z, a->m[3] * v.x + a->m[4] * v.y + a->m[5] * v.z,
             a->m[6] * v.x + a->m[7] * v.y + a->m[8] * v.z);
}
static m3 mm(const m3* a, const m3* b) {
    m3 r;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            double s = 0;
            for (int k = 0; k < 3; k++) s += a->m[3 * i + k] * b->m[3 * k + j];
            r.m[3 * i + j] = s;
        }
    return r;
}
static m3 mt(const m3* a) {
    m3 r;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) r.m[3 * i + j] = a->m[3 * j + i];
    return r;
}
static m3 mf(const float* p) {
    m3 r;
    for (int i = 0; i < 9; i++) r.m[i] = p[i];
    return r;
}
static m3 axis_rot(int axis, double q) {
    double c = cos(q), s = sin(q);
    m3 r = {{1, 0, 0, 0, 1, 0, 0, 0, 1}};
    if (axis == 0) { r.m[4] = c; r.m[5] = -s; r.m[7] = s; r.m[8] = c; }
    else if (axis == 1) { r.m[0] = c; r.m[2] = s; r.m[6] = -s; r.m[8] = c; }
    else { r.m[0] = c; r.m[1] = -s; r.m[3] = s; r.m[4] = c; }
    return r;
}
/* rotation matrix -> xyzw quaternion, w >= 0 */
static void rot_to_quat(const m3* r, double q[4]) {
    double tr = r->m[0] + r->m[4] + r->m[8];
    double x, y, z, w;
    if (tr > 0) {
        double s = sqrt(tr + 1.0) * 2;
        w = 0.25 * s; x = (r->m[7] - r->m[5]) / s; y = (r->m[2] - r->m[6]) / s; z = (r->m[3] - r->m[1]) / s;
    } else if (r->m[0] > r->m[4] && r->m[0] > r->m[8]) {
        double s = sqrt(1.0 + r->m[0] - r->m[4] - r->m[8]) * 2;
        w = (r->m[7] - r->m[5]) / s; x = 0.25 * s; y = (r->m[1] + r->m[3]) / s; z = (r->m[2] + r->m[6]) / s;
    } else if (r->m[4] > r->m[8]) {
        double s = sqrt(1.0 + r->m[4] - r->m[0] - r->m[8]) * 2;
        w = (r->m[2] - r->m[6]) / s; x = (r->m[1] + r->m[3]) / s; y = 0.25 * s; z = (r->m[5] + r->m[7]) / s;
    } else {
        double s = sqrt(1.0 + r->m[8] - r->m[0] - r->m[4]) * 2;
        w = (r->m[3] - r->m[1]) / s; x = (r->m[2] + r->m[6]) / s; y = (r->m[5] + r->m[7]) / s; z = 0.25 * s;
    }
    if (w < 0) { x = -x; y = -y; z = -z; w = -w; }
    q[0] = x; q[1] = y; q[2] = z; q[3] = w;
}

/* ------------------------------------------------------------------------ RNG
 * Counter-based, keyed by (seed, global env id, episode index, draw index).
 * The reference draws from Python's global `random` sequentially on the host
 * (TT:307-312,857-859), which no vectorised implementation can reproduce; the
 * parity tests inject serve velocities instead (ppenv_set_serve_override). */
static uint64_t mix64(uint64_t z) {
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27; z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}
static uint32_t hash32(uint32_t x) {   /* "lowbias32" avalanche hash */
    x ^= x >> 16; x *= 0x7FEB352Du;
    x ^= x >> 15; x *= 0x846CA68Bu;
    x ^= x >> 16;
    return x;
}
static float rng_uniform(uint64_t seed, uint32_t gid, uint32_t episode, uint32_t k) {
    uint32_t h = hash32(gid ^ (uint32_t)seed);
    h = hash32(h + episode * 0x9E3779B9u + (uint32_t)(seed >> 32));
    h = hash32(h + (k + 1u) * 0x85EBCA6Bu);
    return (float)(h >> 8) * (1.0f / 16777216.0f);
}
/* generate_random_speed_for_ball from its three draws (speed, tilt, tilt_z; degrees; the reference's draw order), in the
 * reference's double arithmetic: T3:289-305, TT:296-323, TN:301-328, T4:299-326 (= TT), TA:346-377 (= TN's form; `form` is a
 * PPENV_VARIANT_* value).  Pinned by tests/golden/serve_draws.npz (the reference functions with random.uniform scripted). */
static void serve_from_draws(int form, double speed, double tilt_deg, double tilt_z_deg, float out[3]) {
    double a = tilt_deg * (M_PI / 180.0), az = tilt_z_deg * (M_PI / 180.0);
    if (form == PPENV_VARIANT_T3) {            /* T3:296-300 */
        double s = -speed;
        out[0] = (float)(s * cos(a)); out[1] = (float)(s * sin(a)); out[2] = 0.0f;
    } else if (form == PPENV_VARIANT_TT || form == PPENV_VARIANT_T4) {   /* TT:307-318 = T4:310-321 (sic: sin a sin az, then sin a) */
        double s = -speed;
        out[0] = (float)(s * cos(a) * cos(az)); out[1] = (float)(s * sin(a) * sin(az)); out[2] = (float)(s * sin(a));
    } else {                                         /* TN:312-323 */
        double s = speed;
        out[0] = (float)(-s * cos(a) * cos(az)); out[1] = (float)(s * sin(a) * cos(az)); out[2] = (float)(s * sin(az));
    }
}
static void serve_velocity(const ppenv_config* c, uint32_t gid, uint32_t episode, float out[3]) {
    float u0 = rng_uniform(c->seed, gid, episode, 0);
    float u1 = rng_uniform(c->seed, gid, episode, 1);
    float u2 = rng_uniform(c->seed, gid, episode, 2);
    double speed = c->serve_speed_lo + (c->serve_speed_hi - c->serve_speed_lo) * u0;
    double a = c->serve_tilt_lo_deg + (c->serve_tilt_hi_deg - c->serve_tilt_lo_deg) * u1;
    double az = c->serve_tilt_z_lo_deg + (c->serve_tilt_z_hi_deg - c->serve_tilt_z_lo_deg) * u2;
    serve_from_draws(c->variant, speed, a, az, out);
}
/* pre_physics_step's action -> PD target: TT:1008 with offset / scale TT:664-665 (float32 numpy there), after upstream
 * VecTask.step's clamp to clipActions.  Pinned by tests/golden/pre_physics.npz (the reference's own pre_physics_step). */
static float pd_target(float action, float lo, float hi, float clip) {
    float a = fminf(fmaxf(action, -clip), clip);
    float off = 0.5f * (hi + lo), scale = 0.5f * (hi - lo);   /* TT:664-665 */
    return off + scale * a;                                    /* TT:1008 */
}

/* ------------------------------------------------------- arm kinematics (world) */
typedef struct {
    m3 R[ND];      /* world <- link */
    v3 p[ND];      /* link origin, world */
    v3 z[ND];      /* joint axis, world */
    v3 w[ND];      /* angular velocity, world */
    v3 v[ND];      /* linear velocity of link origin, world */
} arm_fk;

/* the chain base: humanoid 1's torso frame, or humanoid 2's for the 4-actor variant */
typedef struct { const float* rot; const float* pos; } arm_base;
static arm_base base_of(const ppenv_config* c, int arm) {
    arm_base b = {arm == 0 ? c->base_rot : c->base2_rot, arm == 0 ? c->base_pos : c->base2_pos};
    return b;
}
static void arm_forward_kinematics_b(const ppenv_config* c, arm_base base, const double* q, const double* qd, arm_fk* k) {
    m3 Rp = mf(base.rot);
    v3 pp = vf(base.pos), wp = V(0, 0, 0), vp = V(0, 0, 0);
    for (int i = 0; i < ND; i++) {
        const ppenv_joint* j = &c->joint[i];
        m3 R0 = mf(j->origin_rot), Rq = axis_rot(j->axis, q[i]);
        m3 E = mm(&R0, &Rq);
        v3 d = mv(&Rp, vf(j->origin_xyz));
        k->p[i] = vadd(pp, d);
        k->R[i] = mm(&Rp, &E);
        v3 e = V(j->axis == 0, j->axis == 1, j->axis == 2);
        k->z[i] = mv(&k->R[i], e);
        k->v[i] = vadd(vp, vcross(wp, d));
        k->w[i] = vadd(wp, vscale(k->z[i], qd[i]));
        Rp = k->R[i]; pp = k->p[i]; wp = k->w[i]; vp = k->v[i];
    }
}

static void arm_forward_kinematics(const ppenv_config* c, const double* q, const double* qd, arm_fk* k) {
    arm_forward_kinematics_b(c, base_of(c, 0), q, qd, k);
}

/* Recursive Newton-Euler, world coordinates: tau = RNEA(q, qd, qdd) with gravity
 * folded in as a base acceleration of -g when grav != 0. */
static void arm_rnea_b(const ppenv_config* c, arm_base base, const arm_fk* k, const double* qd, const double* qdd, double grav,
                       int use_vel, double* tau) {
    v3 alpha[ND], acc[ND], F[ND], N[ND], comw[ND];
    v3 wp = V(0, 0, 0), alp = V(0, 0, 0), ap = V(0, 0, grav), pp = vf(base.pos); /* base accelerates up by |g| */
    for (int i = 0; i < ND; i++) {
        const ppenv_joint* j = &c->joint[i];
        v3 d = vsub(k->p[i], pp);
        v3 wi = use_vel ? k->w[i] : V(0, 0, 0);
        double qdi = use_vel ? qd[i] : 0.0;
        alpha[i] = vadd(vadd(alp, vscale(k->z[i], qdd[i])), vcross(wp, vscale(k->z[i], qdi)));
        acc[i] = vadd(vadd(ap, vcross(alp, d)), vcross(wp, vcross(wp, d)));
        comw[i] = mv(&k->R[i], vf(j->com));
        v3 ac = vadd(vadd(acc[i], vcross(alpha[i], comw[i])), vcross(wi, vcross(wi, comw[i])));
        m3 I = {{j->inertia[0], j->inertia[3], j->inertia[4], j->inertia[3], j->inertia[1], j->inertia[5],
                 j->inertia[4], j->inertia[5], j->inertia[2]}};
        m3 Rt = mt(&k->R[i]);
        m3 RI = mm(&k->R[i], &I);
        m3 Iw = mm(&RI, &Rt);
        F[i] = vscale(ac, j->mass);
        N[i] = vadd(mv(&Iw, alpha[i]), vcross(wi, mv(&Iw, wi)));
        wp = wi; alp = alpha[i]; ap = acc[i]; pp = k->p[i];
    }
    v3 f = V(0, 0, 0), n = V(0, 0, 0); /* force / moment (about origin of link i) transmitted through joint i */
    for (int i = ND - 1; i >= 0; i--) {
        if (i < ND - 1) n = vadd(n, vcross(vsub(k->p[i + 1], k->p[i]), f)); /* shift child's moment to this origin */
        f = vadd(f, F[i]);
        n = vadd(n, vadd(N[i], vcross(comw[i], F[i])));
        tau[i] = vdot(k->z[i], n);
    }
}

static void arm_rnea(const ppenv_config* c, const arm_fk* k, const double* qd, const double* qdd, double grav, int use_vel, double* tau) {
    arm_rnea_b(c, base_of(c, 0), k, qd, qdd, grav, use_vel, tau);
}

/* qdd from (M + diag(arm)) qdd = tau - C */
static void arm_forward_dynamics_b(const ppenv_config* c, arm_base base, const arm_fk* k, const double* qd, const double* tau,
                                   const double* arm_eff, double* qdd) {
    double C[ND], zero[ND] = {0}, M[ND][ND + 1], col[ND], unit[ND];
    arm_rnea_b(c, base, k, qd, zero, -(double)c->gravity_z, 1, C);
    for (int j = 0; j < ND; j++) {
        memset(unit, 0, sizeof unit);
        unit[j] = 1.0;
        arm_rnea_b(c, base, k, qd, unit, 0.0, 0, col);
        for (int i = 0; i < ND; i++) M[i][j] = col[i];
    }
    for (int i = 0; i < ND; i++) { M[i][i] += arm_eff[i]; M[i][ND] = tau[i] - C[i]; }
    for (int p = 0; p < ND; p++) { /* Gaussian elimination with partial pivoting */
        int best = p;
        for (int r = p + 1; r < ND; r++) if (fabs(M[r][p]) > fabs(M[best][p])) best = r;
        if (best != p) for (int cidx = 0; cidx <= ND; cidx++) { double t = M[p][cidx]; M[p][cidx] = M[best][cidx]; M[best][cidx] = t; }
        for (int r = p + 1; r < ND; r++) {
            double fct = M[r][p] / M[p][p];
            for (int cidx = p; cidx <= ND; cidx++) M[r][cidx] -= fct * M[p][cidx];
        }
    }
    for (int i = ND - 1; i >= 0; i--) {
        double s = M[i][ND];
        for (int j = i + 1; j < ND; j++) s -= M[i][j] * qdd[j];
        qdd[i] = s / M[i][i];
    }
}
static void arm_forward_dynamics(const ppenv_config* c, const arm_fk* k, const double* qd, const double* tau,
                                 const double* arm_eff, double* qdd) {
    arm_forward_dynamics_b(c, base_of(c, 0), k, qd, tau, arm_eff, qdd);
}

/* world pose / velocity of a frame attached to a chain link (or static) */
static void frame_state(const ppenv_config* c, const arm_fk* k, const ppenv_frame* f, v3* pos, m3* rot, v3* lin, v3* ang) {
    m3 Rf = mf(f->rot);
    if (f->link < 0) {
        *pos = vf(f->xyz); *rot = Rf; *lin = V(0, 0, 0); *ang = V(0, 0, 0);
        return;
    }
    (void)c;
    v3 off = mv(&k->R[f->link], vf(f->xyz));
    *pos = vadd(k->p[f->link], off);
    *rot = mm(&k->R[f->link], &Rf);
    *ang = k->w[f->link];
    *lin = vadd(k->v[f->link], vcross(k->w[f->link], off));
}

/* ---------------------------------------------------------------- ball contacts */
typedef struct { v3 p, v, w; } ball_t;

/* Resolve one contact: n = unit normal surface -> ball, s = separation, u = surface velocity. */
static void contact_resolve(const ppenv_config* c, ball_t* b, v3 n, double s, v3 u, double e, double mu, double hb) {
    if (!(s < c->contact_offset)) return;
    double r = c->ball_radius, kappa = c->ball_inertia_factor;
    v3 vrel = vsub(vadd(b->v, vcross(b->w, vscale(n, -r))), u);
    double vn = vdot(vrel, n);
    if (vn < 0) {
        double e_eff = (-vn > c->bounce_threshold) ? e : 0.0;
        double jn = -(1.0 + e_eff) * vn;
        v3 vt = vsub(vrel, vscale(n, vn));
        double vtl = vnorm(vt);
        double jt = 0;
        v3 dir = V(0, 0, 0);
        if (vtl > 1e-9) {
            dir = vscale(vt, 1.0 / vtl);
            double stick = vtl / (1.0 + 1.0 / kappa);
            jt = mu * jn < stick ? mu * jn : stick;
        }
        b->v = vadd(b->v, vsub(vscale(n, jn), vscale(dir, jt)));
        b->w = vadd(b->w, vscale(vcross(n, dir), jt / (kappa * r)));
    }
    if (s < 0) {
        double push = -s, cap = c->max_depenetration_velocity * hb;
        b->p = vadd(b->p, vscale(n, push < cap ? push : cap));
    }
}
static double clampd(double x, double lo, double hi) { return x < lo ? lo : (x > hi ? hi : x); }

static void contact_box(const ppenv_config* c, ball_t* b, const ppenv_box* box, double hb) {
    v3 d = vsub(b->p, vf(box->center));
    v3 h = vf(box->half);
    v3 q = V(clampd(d.x, -h.x, h.x), clampd(d.y, -h.y, h.y), clampd(d.z, -h.z, h.z));
    v3 diff = vsub(d, q);
    double dist = vnorm(diff);
    v3 n; double s;
    if (dist > 1e-12) { n = vscale(diff, 1.0 / dist); s = dist - c->ball_radius; }
    else { /* centre inside the box: leave through the nearest face */
        double px = h.x - fabs(d.x), py = h.y - fabs(d.y), pz = h.z - fabs(d.z);
        if (px <= py && px <= pz) { n = V(d.x >= 0 ? 1 : -1, 0, 0); s = -px - c->ball_radius; }
        else if (py <= pz) { n = V(0, d.y >= 0 ? 1 : -1, 0); s = -py - c->ball_radius; }
        else { n = V(0, 0, d.z >= 0 ? 1 : -1); s = -pz - c->ball_radius; }
    }
    contact_resolve(c, b, n, s, V(0, 0, 0), box->restitution, box->friction, hb);
}
static void contact_capsule(const ppenv_config* c, ball_t* b, v3 a, v3 bb, v3 ua, v3 ub, double radius, double e,
                            double mu, double hb) {
    v3 ab = vsub(bb, a);
    double l2 = vdot(ab, ab), t = 0;
    if (l2 > 1e-12) t = clampd(vdot(vsub(b->p, a), ab) / l2, 0, 1);
    v3 cp = vadd(a, vscale(ab, t));
    v3 diff = vsub(b->p, cp);
    double dist = vnorm(diff);
    v3 n = dist > 1e-12 ? vscale(diff, 1.0 / dist) : V(0, 0, 1);
    v3 u = vadd(ua, vscale(vsub(ub, ua), t));
    contact_resolve(c, b, n, dist - radius - c->ball_radius, u, e, mu, hb);
}
/* solid disc (flat cylinder): centre cc, unit axis nn, linear velocity uc of the centre, axis rate nd */
static void contact_disc(const ppenv_config* c, ball_t* b, v3 cc, v3 nn, v3 uc, v3 nd, double hb) {
    double R = c->paddle_radius, tp = c->paddle_half_thickness;
    v3 d = vsub(b->p, cc);
    double hgt = vdot(d, nn);
    v3 radial = vsub(d, vscale(nn, hgt));
    double rr = vnorm(radial);
    v3 n, closest; double s;
    if (fabs(hgt) < tp && rr < R) { /* centre inside the blade: leave through the nearer face */
        double sg = hgt >= 0 ? 1.0 : -1.0;
        n = vscale(nn, sg);
        s = -(tp - fabs(hgt)) - c->ball_radius;
        closest = vadd(cc, vadd(vscale(nn, sg * tp), radial));
    } else {
        double hc = clampd(hgt, -tp, tp);
        double rc = rr < R ? rr : R;
        v3 rdir = rr > 1e-12 ? vscale(radial, rc / rr) : V(0, 0, 0);
        closest = vadd(cc, vadd(vscale(nn, hc), rdir));
        v3 diff = vsub(b->p, closest);
        double dist = vnorm(diff);
        n = dist > 1e-12 ? vscale(diff, 1.0 / dist) : nn;
        s = dist - c->ball_radius;
    }
    v3 omega_perp = vcross(nn, nd);
    v3 u = vadd(uc, vcross(omega_perp, vsub(closest, cc)));
    contact_resolve(c, b, n, s, u, c->paddle_restitution, c->paddle_friction, hb);
}

/* collision geometry of the arm at the start of a substep: points and their velocities */
typedef struct {
    v3 pc, pn, vpc, pnd;          /* paddle centre, axis, centre velocity, axis rate (omega x n) */
    v3 sa[PPENV_MAX_SHAPES], sb[PPENV_MAX_SHAPES], va[PPENV_MAX_SHAPES], vb[PPENV_MAX_SHAPES];
} arm_geom;

static void link_point_state(const arm_fk* k, int link, const float* local, v3* p, v3* v) {
    if (link < 0) { *p = vf(local); *v = V(0, 0, 0); return; }
    v3 off = mv(&k->R[link], vf(local));
    *p = vadd(k->p[link], off);
    *v = vadd(k->v[link], vcross(k->w[link], off));
}
static void arm_geometry_s(const ppenv_config* c, const ppenv_shape* shapes, const arm_fk* k, arm_geom* g) {
    link_point_state(k, c->paddle_link, c->paddle_center, &g->pc, &g->vpc);
    g->pn = mv(&k->R[c->paddle_link], vf(c->paddle_normal));
    g->pnd = vcross(k->w[c->paddle_link], g->pn);
    for (int s = 0; s < c->num_shapes; s++) {
        link_point_state(k, shapes[s].link, shapes[s].a, &g->sa[s], &g->va[s]);
        link_point_state(k, shapes[s].link, shapes[s].b, &g->sb[s], &g->vb[s]);
    }
}
static void arm_geometry(const ppenv_config* c, const arm_fk* k, arm_geom* g) { arm_geometry_s(c, c->shape, k, g); }

/* One substep of the ball.  The arm's shapes move linearly from their pose at the START of the substep with
 * the velocities they have there (contacts are generated from start-of-step poses, as PhysX does); within the
 * substep the ball and the arm therefore do not depend on each other. */
static void ball_substep_nb(const ppenv_config* c, ball_t* b, double quat[4], int narms, const arm_geom* const* garr, const v3* bounds, double h) {
    int M = c->ball_substeps;
    double hb = h / M;
    for (int m = 0; m < M; m++) {
        double t = (double)m / M * h;
        b->v.z += c->gravity_z * hb;
        double damp = 1.0 - c->ball_angular_damping * hb;
        b->w = vscale(b->w, damp > 0 ? damp : 0);
        /* ground */
        contact_resolve(c, b, V(0, 0, 1), b->p.z - c->ground_z - c->ball_radius, V(0, 0, 0), c->ground_restitution,
                        c->ground_friction, hb);
        contact_box(c, b, &c->table, hb);
        contact_box(c, b, &c->net, hb);
        for (int arm = 0; arm < narms; arm++) {   /* humanoid 1's shapes, then humanoid 2's (4-actor variant) */
            const arm_geom* g = garr[arm];
            const float* bound = arm == 0 ? c->humanoid_bound_center : c->humanoid2_bound_center;
            const ppenv_shape* shapes = arm == 0 ? c->shape : c->shape2;
            v3 bc = bounds ? bounds[arm] : vf(bound);   /* the 27-DoF humanoid's bound follows its torso */
            if (!(vnorm(vsub(b->p, bc)) < c->humanoid_bound_radius)) continue;
            v3 cc = vadd(g->pc, vscale(g->vpc, t));
            v3 nn = vadd(g->pn, vscale(g->pnd, t));
            nn = vscale(nn, 1.0 / vnorm(nn));
            contact_disc(c, b, cc, nn, g->vpc, g->pnd, hb);
            for (int s = 0; s < c->num_shapes; s++) {
                const ppenv_shape* sh = &shapes[s];
                v3 a = vadd(g->sa[s], vscale(g->va[s], t)), bb = vadd(g->sb[s], vscale(g->vb[s], t));
                contact_capsule(c, b, a, bb, g->va[s], g->vb[s], sh->radius, sh->restitution, sh->friction, hb);
            }
        }
        b->p = vadd(b->p, vscale(b->v, hb));
    }
    /* orientation: q <- normalize(q + h/2 * (w,0) (x) q), xyzw */
    double wx = b->w.x, wy = b->w.y, wz = b->w.z, x = quat[0], y = quat[1], z = quat[2], w = quat[3];
    double dx = 0.5 * h * (wx * w + wy * z - wz * y);
    double dy = 0.5 * h * (wy * w + wz * x - wx * z);
    double dz = 0.5 * h * (wz * w + wx * y - wy * x);
    double dw = 0.5 * h * (-wx * x - wy * y - wz * z);
    x += dx; y += dy; z += dz; w += dw;
    double nrm = sqrt(x * x + y * y + z * z + w * w);
    quat[0] = x / nrm; quat[1] = y / nrm; quat[2] = z / nrm; quat[3] = w / nrm;
}

static void ball_substep_n(const ppenv_config* c, ball_t* b, double quat[4], int narms, const arm_geom* const* garr, double h) {
    ball_substep_nb(c, b, quat, narms, garr, NULL, h);
}
static void ball_substep(const ppenv_config* c, ball_t* b, double quat[4], const arm_geom* g, double h) {
    ball_substep_n(c, b, quat, 1, &g, h);
}

/* ------------------------------------------------------ fp32 reward / obs / reset */
/* my_quat_rotate (torch_jit_utils): a = v (2 w^2 - 1), b = 2 w (qv x v), c = 2 qv (qv . v) */
static void quat_rotate_f(const float q[4], const float v[3], float out[3]) {
    float qw = q[3];
    float s = 2.0f * (qw * qw) - 1.0f;
    float cx = q[1] * v[2] - q[2] * v[1], cy = q[2] * v[0] - q[0] * v[2], cz = q[0] * v[1] - q[1] * v[0];
    float dot = q[0] * v[0] + q[1] * v[1] + q[2] * v[2];
    out[0] = v[0] * s + cx * qw * 2.0f + q[0] * dot * 2.0f;
    out[1] = v[1] * s + cy * qw * 2.0f + q[1] * dot * 2.0f;
    out[2] = v[2] * s + cz * qw * 2.0f + q[2] * dot * 2.0f;
}
/* calc_heading_quat_inv (torch_jit_utils) */
static void heading_quat_inv_f(const float q[4], float out[4]) {
    float ref[3] = {1.0f, 0.0f, 0.0f}, rd[3];
    quat_rotate_f(q, ref, rd);
    float heading = atan2f(rd[1], rd[0]);
    float theta = (-heading) / 2.0f;
    float xyz2 = sinf(theta), w = cosf(theta);
    float nrm = sqrtf(xyz2 * xyz2 + w * w);
    if (nrm < 1e-9f) nrm = 1e-9f;
    out[0] = 0.0f / nrm; out[1] = 0.0f / nrm; out[2] = xyz2 / nrm; out[3] = w / nrm;
}

/* observed body states for one env: [NB][13] pos3 quat4 lin3 ang3 */
typedef float bodies_t[NB][13];

/* compute_observations: TT:770-799 -> 1640-1708 */
static void compute_obs(const bodies_t bs, const float* dof_pos, const float* dof_vel, const float* ball, float* obs) {
    const float* root_pos = &bs[0][0];
    float hinv[4];
    heading_quat_inv_f(&bs[0][3], hinv);
    for (int j = 0; j < NB; j++) {   /* TT:1696-1697 */
        float rel[3] = {bs[j][0] - root_pos[0], bs[j][1] - root_pos[1], bs[j][2] - root_pos[2]};
        quat_rotate_f(hinv, rel, &obs[3 * j]);
        quat_rotate_f(hinv, &bs[j][7], &obs[3 * NB + 3 * j]);
    }
    for (int d = 0; d < ND; d++) {   /* TT:1702-1703 */
        obs[6 * NB + d] = dof_pos[d];
        obs[6 * NB + ND + d] = dof_vel[d] * 0.1f;
    }
    float rel[3] = {ball[0] - root_pos[0], ball[1] - root_pos[1], ball[2] - root_pos[2]};
    quat_rotate_f(hinv, rel, &obs[6 * NB + 2 * ND]);          /* TT:1657-1660 */
    quat_rotate_f(hinv, &ball[7], &obs[6 * NB + 2 * ND + 3]);
}

static float power_term(const float* dof_force, const float* dof_vel, int ndof) {
    float p = 0.0f;
    for (int d = 0; d < ndof; d++) p += fabsf(dof_force[d] * dof_vel[d]);
    return p;
}

/* Reward + reset decision for one env.  Inputs are the post-step, pre-reset
 * state; flags are read-modify-write (sticky).  Returns reward, *reset_out 0/1. */
static float compute_reward(const ppenv_config* c, float humanoid_x, const float* paddle_pos, float pre_vx,
                            const float* ball, float power, int64_t progress, uint32_t* flags, int64_t* reset_out) {
    const float Bx = ball[0], By = ball[1], Bz = ball[2], vx = ball[7];
    const float alpha = c->alpha_velocity_reward, penalty = c->penalty;
    const float threshold = 0.1f;
    float power_reward = -c->power_coefficient * power;   /* power = sum_j |dof_force_j * dof_vel_j| (TT:1246) */
    uint32_t f = *flags;
    float reward;
    int64_t die = 0;
    if (c->variant == PPENV_VARIANT_T3) {                   /* T3:1080-1173 */
        float dx = paddle_pos[0] - Bx, dy = paddle_pos[1] - By, dz = paddle_pos[2] - Bz;
        float dist = sqrtf(dx * dx + dy * dy + dz * dz);
        float pos_reward = 1.0f / (1.0f + 1.5f * dist * dist);
        float vel_reward = (pre_vx < 0.0f && vx > 0.0f) ? alpha * fabsf(vx) : 0.0f;      /* T3:1126-1128 */
        reward = pos_reward + power_reward + vel_reward;                                   /* T3:1141 */
        int missed = Bx < paddle_pos[0] - 1e-3f;                                           /* T3:1146 */
        if (missed) reward = reward + penalty;
        if (missed) die = 1;                                                               /* T3:1158 */
        if (Bz < threshold) die = 1;                                                       /* T3:1161 */
    } else if (c->variant == PPENV_VARIANT_TT || c->variant == PPENV_VARIANT_T4) {   /* TT:1105-1270 == T4:1113-1278 */
        float dx = paddle_pos[0] - Bx, dy = paddle_pos[1] - By, dz = paddle_pos[2] - Bz;
        float dist = sqrtf(dx * dx + dy * dy + dz * dz);                                   /* TT:1144-1146 */
        float pos_reward = 1.0f / (1.0f + 1.5f * dist * dist);                             /* TT:1147 */
        int cond = pre_vx < 0.0f && vx > 0.0f;                                             /* TT:1153 */
        float vel_reward = (cond && !(f & PPENV_FLAG_COND_CALC)) ? alpha * fabsf(vx) : 0.0f;   /* TT:1156-1160 */
        if (cond) f |= PPENV_FLAG_COND_CALC;                                               /* TT:1163 */
        int missed = Bx < humanoid_x - 0.05f;                                              /* TT:1169 */
        reward = missed ? 0.0f + penalty : 0.0f;                                           /* TT:1172-1173 */
        int bounce = Bz < 0.83f && vx > 0.0f && By < 0.6f && By > -0.6f;                   /* TT:1184 */
        float hit = 0.0f;
        int early = Bx < 2.44f && bounce;
        if (early && !(f & PPENV_FLAG_REWARD_CALC)) hit = c->not_hit_table_penalty;        /* TT:1187-1191 */
        if (early) f |= PPENV_FLAG_REWARD_CALC;                                            /* TT:1192 */
        if (early) f &= ~PPENV_FLAG_NO_BOUNCE;                                             /* TT:1196 */
        int inx = Bx > 2.44f && Bx < 3.1f;                                                 /* TT:1199 */
        int good = inx && bounce && (f & PPENV_FLAG_NO_BOUNCE);
        if (good && !(f & PPENV_FLAG_REWARD_CALC)) hit = c->hit_table_reward;              /* TT:1201-1205 */
        if (good) f |= PPENV_FLAG_REWARD_CALC;                                             /* TT:1206 */
        if (Bx >= 3.1f && vx > 0.0f && !(f & PPENV_FLAG_REWARD_CALC)) hit = c->not_hit_table_penalty; /* TT:1209-1213 */
        if (Bx >= 3.1f) f |= PPENV_FLAG_REWARD_CALC;                                       /* TT:1214 (no vx guard) */
        float net = (Bx > 1.7f && Bx < 1.8f && vx > 0.0f && By < 0.4f && By > -0.4f && Bz > 0.98f && Bz < 1.14f)
                        ? 400.0f : 0.0f;                                                   /* TT:1226-1244 */
        reward += (((pos_reward + power_reward) + vel_reward) + hit) + net;               /* TT:1251 */
        if (Bz < threshold) die = 1;                                                       /* TT:1263 */
    } else {                                                /* TN:1115-1322 */
        int hit_paddle = pre_vx < 0.0f && vx > 1.0f;                                       /* TN:1160 */
        int missed = (Bx < humanoid_x - 0.05f) || (Bx < paddle_pos[0] - 0.1f);             /* TN:1165 */
        reward = (!(f & PPENV_FLAG_MISSED_CALC) && missed) ? 0.0f + penalty : 0.0f;        /* TN:1172-1176 */
        if (missed) f |= PPENV_FLAG_MISSED_CALC;                                           /* TN:1178 */
        float dy = paddle_pos[1] - By, dz = paddle_pos[2] - Bz;
        float dist = sqrtf(dy * dy + dz * dz);                                             /* TN:1185-1186 */
        float pos_reward = 0.0f;
        if (!(f & PPENV_FLAG_COND_CALC) || (Bx < humanoid_x - 0.05f))
            pos_reward = 1.0f * expf(-20.0f * dist * dist);                                /* TN:1188-1192 */
        float vel_reward = (hit_paddle && !(f & PPENV_FLAG_COND_CALC)) ? alpha * fabsf(vx) : 0.0f;  /* TN:1198-1202 */
        if (hit_paddle) f |= PPENV_FLAG_COND_CALC;                                         /* TN:1204 */
        reward += (pos_reward + power_reward) + vel_reward;                                /* TN:1299 */
        if (Bz < threshold) reward = -800.0f + reward;                                     /* TN:1313-1315 */
        /* no early stop: die stays 0 (TN:1317) */
    }
    *flags = f;
    *reset_out = (progress >= (int64_t)c->max_episode_length - 1) ? 1 : die;  /* TT:1265 */
    return reward;
}

static uint32_t initial_flags(const ppenv_config* c) {
    (void)c;
    return PPENV_FLAG_NO_BOUNCE; /* TT:241-243 / TN:244-248: all False except no_bounce_before_half_mask */
}

/* ------------------------------------------------------------------ lifecycle */
ppo_env* ppo_create(const ppenv_config* cfg) {
    if (!cfg || cfg->abi_version != PPENV_ABI_VERSION || cfg->num_envs <= 0) return NULL;
    ppo_env* e = (ppo_env*)calloc(1, sizeof *e);
    e->cfg = *cfg;
    int n = e->n = cfg->num_envs;
    int A = e->A = cfg->variant == PPENV_VARIANT_T4 ? 2 : 1;
    if (cfg->num_humanoids != A) { free(e); return NULL; }
    e->threads = 1;
    e->obs = (float*)calloc((size_t)n * A * PPENV_NUM_OBS, sizeof(float));
    e->rew = (float*)calloc((size_t)n * A, sizeof(float));
    e->reset = (int64_t*)calloc((size_t)n * A, sizeof(int64_t));
    e->progress = (int64_t*)calloc((size_t)n * A, sizeof(int64_t));
    e->dof_pos = (float*)calloc((size_t)n * A * ND, sizeof(float));
    e->dof_vel = (float*)calloc((size_t)n * A * ND, sizeof(float));
    e->dof_force = (float*)calloc((size_t)n * A * ND, sizeof(float));
    e->ball = (float*)calloc((size_t)n * 13, sizeof(float));
    e->flags = (uint32_t*)calloc((size_t)n * A, sizeof(uint32_t));
    e->episode = (uint32_t*)calloc(n, sizeof(uint32_t));
    e->serve = (float*)calloc((size_t)n * 3, sizeof(float));
    return e;
}
void ppo_destroy(ppo_env* e) {
    if (!e) return;
    free(e->obs); free(e->rew); free(e->reset); free(e->progress); free(e->dof_pos); free(e->dof_vel);
    free(e->dof_force); free(e->ball); free(e->flags); free(e->episode); free(e->serve); free(e->cfg_env); free(e);
}
void ppo_set_threads(ppo_env* e, int t) { e->threads = t > 0 ? t : 1; }

typedef struct ppo_buffers {
    int32_t num_envs, num_agents;
    float* obs_buf; float* rew_buf; int64_t* reset_buf; int64_t* progress_buf;
    float* dof_pos; float* dof_vel; float* dof_force; float* ball;
    uint32_t* flags; uint32_t* episode; float* serve_override;
} ppo_buffers;
void ppo_buffers_of(ppo_env* e, ppo_buffers* b) {
    b->num_envs = e->n; b->num_agents = e->A; b->obs_buf = e->obs; b->rew_buf = e->rew; b->reset_buf = e->reset;
    b->progress_buf = e->progress; b->dof_pos = e->dof_pos; b->dof_vel = e->dof_vel; b->dof_force = e->dof_force;
    b->ball = e->ball; b->flags = e->flags; b->episode = e->episode; b->serve_override = e->serve;
}

static void fresh_serve(ppo_env* e, int i, float v[3]) {
    if (e->serve_on) { for (int k = 0; k < 3; k++) v[k] = e->serve[(size_t)k * e->n + i]; }
    else serve_velocity(&e->cfg, (uint32_t)(e->cfg.env_id_offset + i), e->episode[i], v);
}

/* restore env i's simulation state to the initial one with a fresh serve (TT:853-867) */
static void reset_env_state(ppo_env* e, int i, int reset_dofs) {
    const ppenv_config* c = &e->cfg;
    int n = e->n;
    float v[3];
    fresh_serve(e, i, v);
    for (int k = 0; k < 3; k++) e->ball[(size_t)k * n + i] = c->ball_init_pos[k];
    for (int k = 0; k < 4; k++) e->ball[(size_t)(3 + k) * n + i] = c->ball_init_quat[k];
    for (int k = 0; k < 3; k++) e->ball[(size_t)(7 + k) * n + i] = v[k];
    for (int k = 0; k < 3; k++) e->ball[(size_t)(10 + k) * n + i] = 0.0f;
    if (reset_dofs)
        for (int d = 0; d < e->A * ND; d++) {   /* T4:873: the dof states of both humanoids */
            e->dof_pos[(size_t)d * n + i] = c->init_dof_pos[d % ND];
            e->dof_vel[(size_t)d * n + i] = c->init_dof_vel[d % ND];
        }
}

static void gather_env(const ppo_env* e, int i, float* q, float* qd, float* ball) {   /* q, qd: [A * ND] */
    int n = e->n;
    for (int d = 0; d < e->A * ND; d++) { q[d] = e->dof_pos[(size_t)d * n + i]; qd[d] = e->dof_vel[(size_t)d * n + i]; }
    for (int k = 0; k < 13; k++) ball[k] = e->ball[(size_t)k * n + i];
}

/* xyzw unit quaternion -> rotation matrix */
static m3 quat_to_rot_f(const float* q) {
    double x = q[0], y = q[1], z = q[2], w = q[3];
    m3 r = {{1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z),
             2 * (y * z - x * w), 2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)}};
    return r;
}
/* observed bodies of humanoid `arm` (0: humanoid 1; 1: humanoid 2 of the 4-actor variant, whose pelvis is static at its own root pose) */
static void bodies_from_fk_arm(const ppenv_config* c, int arm, const arm_fk* k, bodies_t bs) {
    for (int j = 0; j < NB; j++) {
        v3 pos, lin, ang; m3 rot; double qt[4];
        frame_state(c, k, &c->obs_body[j], &pos, &rot, &lin, &ang);
        if (arm == 1 && c->obs_body[j].link < 0) { pos = vf(c->humanoid2_root_pos); rot = quat_to_rot_f(c->humanoid2_root_quat); }
        rot_to_quat(&rot, qt);
        bs[j][0] = (float)pos.x; bs[j][1] = (float)pos.y; bs[j][2] = (float)pos.z;
        for (int t = 0; t < 4; t++) bs[j][3 + t] = (float)qt[t];
        bs[j][7] = (float)lin.x; bs[j][8] = (float)lin.y; bs[j][9] = (float)lin.z;
        bs[j][10] = (float)ang.x; bs[j][11] = (float)ang.y; bs[j][12] = (float)ang.z;
    }
}
static void bodies_from_fk(const ppenv_config* c, const arm_fk* k, bodies_t bs) { bodies_from_fk_arm(c, 0, k, bs); }

/* observations of env i from the current SoA state (used by create / reset_all): one row per agent */
static void obs_from_state(ppo_env* e, int i) {
    const ppenv_config* c = &e->cfg;
    float qf[2 * ND], qdf[2 * ND], ball[13];
    gather_env(e, i, qf, qdf, ball);
    for (int a = 0; a < e->A; a++) {
        double q[ND], qd[ND];
        for (int d = 0; d < ND; d++) { q[d] = qf[a * ND + d]; qd[d] = qdf[a * ND + d]; }
        arm_fk k;
        arm_forward_kinematics_b(c, base_of(c, a), q, qd, &k);
        bodies_t bs;
        bodies_from_fk_arm(c, a, &k, bs);
        compute_obs(bs, &qf[a * ND], &qdf[a * ND], ball, &e->obs[((size_t)i * e->A + a) * PPENV_NUM_OBS]);
    }
}

static void init_env(ppo_env* e, int i) {
    reset_env_state(e, i, 1);
    for (int d = 0; d < e->A * ND; d++) e->dof_force[(size_t)d * e->n + i] = 0.0f;
    for (int a = 0; a < e->A; a++) {
        e->flags[(size_t)a * e->n + i] = initial_flags(&e->cfg);
        e->progress[(size_t)i * e->A + a] = 0;
        e->reset[(size_t)i * e->A + a] = 1;  /* upstream VecTask.allocate_buffers: reset_buf = ones; overwritten by the first step (TT:740) */
        e->rew[(size_t)i * e->A + a] = 0.0f;
    }
    obs_from_state(e, i);
}
/* state as after _create_envs (TT:512-643): creation is episode 0 of every env */
void ppo_init(ppo_env* e) {
    for (int i = 0; i < e->n; i++) { e->episode[i] = 0; init_env(e, i); }
}
/* VecTask.reset(): every env back to its initial state with a fresh serve */
void ppo_reset_all(ppo_env* e) {
    for (int i = 0; i < e->n; i++) { e->episode[i] += 1; init_env(e, i); }
}
/* reset_idx(env_ids) -> _reset_idx (TT:809-812, 847-906): only the listed envs; TN keeps its dof state (TN:888-901).
 * The reference leaves obs_buf alone there; refresh_obs rewrites the listed envs' rows from the reset state. */
int ppo_reset_idx(ppo_env* e, const int64_t* ids, int count, int refresh_obs) {
    for (int t = 0; t < count; t++) {
        if (ids[t] < 0 || ids[t] >= e->n) return -1;
        int i = (int)ids[t];
        e->episode[i] += 1;
        reset_env_state(e, i, e->cfg.variant != PPENV_VARIANT_TN);
        for (int a = 0; a < e->A; a++) {
            e->flags[(size_t)a * e->n + i] = initial_flags(&e->cfg);   /* TT:903-905 */
            e->progress[(size_t)i * e->A + a] = 0;                      /* TT:902 */
        }
        if (refresh_obs) obs_from_state(e, i);
    }
    return 0;
}
/* Domain randomisation of the fused 3-actor step (include/ppenv.h ppenv_randomization): per-env tables as host arrays (SoA [rows][N],
 * NULL = not randomised).  The oracle gives every env its own copy of the config with the scales applied. */
int ppo_set_randomization(ppo_env* e, const float* kp_scale, const float* kd_scale, const float* mass_scale, const float* e_scale,
                          const float* mu_scale, float action_sigma, float obs_sigma, int on) {
    free(e->cfg_env);
    e->cfg_env = NULL;
    e->dr_action_sigma = e->dr_obs_sigma = 0.f;
    if (!on) return 0;
    /* two humanoids (the 4-actor variant): both are instances of the one "humanoid" actor of the yaml's randomization_params, so an env's table entries
     * apply to both of its arms and to both shape sets */
    e->dr_action_sigma = action_sigma; e->dr_obs_sigma = obs_sigma;
    if (!kp_scale && !kd_scale && !mass_scale && !e_scale && !mu_scale) return 0;
    int n = e->n;
    e->cfg_env = (ppenv_config*)malloc((size_t)n * sizeof(ppenv_config));
    if (!e->cfg_env) return -2;
    for (int i = 0; i < n; i++) {
        ppenv_config* c = &e->cfg_env[i];
        *c = e->cfg;
        for (int d = 0; d < ND; d++) {
            if (kp_scale) c->joint[d].kp *= kp_scale[(size_t)d * n + i];
            if (kd_scale) c->joint[d].kd *= kd_scale[(size_t)d * n + i];
            if (mass_scale) {
                float s = mass_scale[(size_t)d * n + i];
                c->joint[d].mass *= s;
                for (int k = 0; k < 6; k++) c->joint[d].inertia[k] *= s;
            }
        }
        float es = e_scale ? e_scale[i] : 1.f, fs = mu_scale ? mu_scale[i] : 1.f;
        c->paddle_restitution = fminf(c->paddle_restitution * es, c->restitution_max); c->paddle_friction *= fs;
        for (int s = 0; s < c->num_shapes; s++) { c->shape[s].restitution = fminf(c->shape[s].restitution * es, c->restitution_max); c->shape[s].friction *= fs; }
        if (e->A == 2)
            for (int s = 0; s < c->num_shapes; s++) { c->shape2[s].restitution = fminf(c->shape2[s].restitution * es, c->restitution_max); c->shape2[s].friction *= fs; }
    }
    return 0;
}
void ppo_set_gravity(ppo_env* e, float gz) {
    e->cfg.gravity_z = gz;
    if (e->cfg_env) for (int i = 0; i < e->n; i++) e->cfg_env[i].gravity_z = gz;
}
void ppo_set_serve_override(ppo_env* e, const float* serve /* [N,3] */, int on) {
    e->serve_on = on;
    if (on && serve)
        for (int i = 0; i < e->n; i++)
            for (int k = 0; k < 3; k++) e->serve[(size_t)k * e->n + i] = serve[(size_t)i * 3 + k];
}

/* -------------------------------------------------------------------- the step */
/* additive Gaussian white noise of the domain randomisation (yaml:106-113): Box-Muller on two counter-RNG draws keyed by
 * (seed, global env id, episode, progress * 256 + index).  Indices 2 j and 2 j + 1 share their (u1, u2) and take the cosine / the sine branch,
 * as in the kernel (ppenv_device.h dr_gauss_pair); libm here, the hardware's log2 / sqrt / sin / cos there: the device is within 5.0e-7 of a
 * unit normal of Box-Muller in double (measured, tests/test_rng_streams_gpu.py). */
static float dr_gauss(uint64_t seed, uint32_t gid, uint32_t episode, uint32_t progress, uint32_t index) {
    uint32_t k = progress * 256u + (index & ~1u);
    float u1 = rng_uniform(seed ^ 0x5DEECE66Dull, gid, episode, 2u * k), u2 = rng_uniform(seed ^ 0x5DEECE66Dull, gid, episode, 2u * k + 1u);
    float rad = sqrtf(-2.0f * logf(fmaxf(u1, 5.9604645e-8f)));
    return (index & 1u) ? rad * sinf(6.2831853f * u2) : rad * cosf(6.2831853f * u2);
}

static void step_env(ppo_env* e, int i, const float* actions) {
    const ppenv_config* c = e->cfg_env ? &e->cfg_env[i] : &e->cfg;      /* domain randomisation: this env's own scaled model */
    int n = e->n;
    float qf[ND], qdf[ND], ballf[13];
    gather_env(e, i, qf, qdf, ballf);
    const uint32_t dr_gid = (uint32_t)(c->env_id_offset + i), dr_ep = e->episode[i], dr_prog = (uint32_t)e->progress[i];

    /* pre_physics_step: TT:1003-1020 (clamp is VecTask.step, clipActions) */
    double target[ND];
    for (int d = 0; d < ND; d++) {
        float act = actions[(size_t)i * ND + d];
        if (e->dr_action_sigma > 0.f) act += e->dr_action_sigma * dr_gauss(c->seed, dr_gid, dr_ep, dr_prog, (uint32_t)d);   /* before the clamp, as upstream VecTask.step */
        target[d] = pd_target(act, c->joint[d].lower, c->joint[d].upper, c->clip_actions);   /* TT:1008 */
    }
    float pre_vx = ballf[7];                                        /* TT:1020 */

    /* gym.simulate: `substeps` substeps of the build's physics specification */
    double q[ND], qd[ND], tau_drive[ND] = {0};
    for (int d = 0; d < ND; d++) { q[d] = qf[d]; qd[d] = qdf[d]; }
    ball_t b = {vf(&ballf[0]), vf(&ballf[7]), vf(&ballf[10])};
    double bq[4] = {ballf[3], ballf[4], ballf[5], ballf[6]};
    double h = (double)c->dt / c->substeps;
    arm_fk k0, k1;
    arm_forward_kinematics(c, q, qd, &k0);
    for (int s = 0; s < c->substeps; s++) {
        double tau[ND], arm_eff[ND], qdd[ND];
        for (int d = 0; d < ND; d++) {   /* implicit PD, explicit part clamped to the effort limit (continuous at saturation) */
            const ppenv_joint* j = &c->joint[d];
            double err = target[d] - q[d];
            tau[d] = clampd(j->kp * (err - h * qd[d]) - j->kd * qd[d], -j->effort, j->effort);
            arm_eff[d] = j->armature + h * j->kd + h * h * j->kp;
        }
        arm_forward_dynamics(c, &k0, qd, tau, arm_eff, qdd);
        for (int d = 0; d < ND; d++) {
            const ppenv_joint* j = &c->joint[d];
            double err = target[d] - q[d];
            double v_new = qd[d] + h * qdd[d];
            tau_drive[d] = clampd(j->kp * (err - h * v_new) - j->kd * v_new, -j->effort, j->effort);   /* reported within the limit */
            v_new = clampd(v_new, -j->vel_limit, j->vel_limit);
            double q_new = q[d] + h * v_new;
            if (q_new > j->upper) { q_new = j->upper; if (v_new > 0) v_new = 0; }
            if (q_new < j->lower) { q_new = j->lower; if (v_new < 0) v_new = 0; }
            q[d] = q_new; qd[d] = v_new;
        }
        arm_geom g;
        arm_geometry(c, &k0, &g);              /* pose and velocities at the start of the substep */
        ball_substep(c, &b, bq, &g, h);
        arm_forward_kinematics(c, q, qd, &k1);
        k0 = k1;
    }

    /* refresh_sim_tensors (TT:801-807): round the state to the fp32 tensors */
    float dof_force[ND];
    for (int d = 0; d < ND; d++) { qf[d] = (float)q[d]; qdf[d] = (float)qd[d]; dof_force[d] = (float)tau_drive[d]; }
    ballf[0] = (float)b.p.x; ballf[1] = (float)b.p.y; ballf[2] = (float)b.p.z;
    for (int t = 0; t < 4; t++) ballf[3 + t] = (float)bq[t];
    ballf[7] = (float)b.v.x; ballf[8] = (float)b.v.y; ballf[9] = (float)b.v.z;
    ballf[10] = (float)b.w.x; ballf[11] = (float)b.w.y; ballf[12] = (float)b.w.z;
    bodies_t bs;
    bodies_from_fk(c, &k0, bs);

    /* post_physics_step: TT:1022-1039 */
    int64_t progress = e->progress[i] + 1;                          /* TT:1023 */
    uint32_t flags = e->flags[i];
    int64_t reset;
    float rew = compute_reward(c, c->humanoid_root_pos[0], bs[c->paddle_obs_index], pre_vx, ballf, power_term(dof_force, qdf, ND),
                               progress, &flags, &reset);
    for (int d = 0; d < ND; d++) {
        e->dof_pos[(size_t)d * n + i] = qf[d]; e->dof_vel[(size_t)d * n + i] = qdf[d];
        e->dof_force[(size_t)d * n + i] = dof_force[d];
    }
    for (int t = 0; t < 13; t++) e->ball[(size_t)t * n + i] = ballf[t];
    if (reset) {                                                    /* TT:1034-1036 -> 847-906 */
        e->episode[i] += 1;
        reset_env_state(e, i, c->variant != PPENV_VARIANT_TN);      /* TN:888-901 keeps the dof state */
        progress = 0;                                               /* TT:902 */
        flags = initial_flags(c);                                   /* TT:903-905 */
        gather_env(e, i, qf, qdf, ballf);
    }
    e->progress[i] = progress; e->flags[i] = flags; e->rew[i] = rew; e->reset[i] = reset;
    /* TT:1039: dof / ball already show the reset state, body states are the pre-reset ones */
    compute_obs(bs, qf, qdf, ballf, &e->obs[(size_t)i * PPENV_NUM_OBS]);
    if (e->dr_obs_sigma > 0.f)
        for (int k = 0; k < PPENV_NUM_OBS; k++) e->obs[(size_t)i * PPENV_NUM_OBS + k] += e->dr_obs_sigma * dr_gauss(c->seed, dr_gid, dr_ep, dr_prog, 16u + (uint32_t)k);
}

static void step_env_t4(ppo_env* e, int i, const float* actions);

void ppo_step(ppo_env* e, const float* actions) {
    int n = e->n;
#ifdef _OPENMP
#pragma omp parallel for num_threads(e->threads) schedule(static)
#endif
    for (int i = 0; i < n; i++) {
        if (e->A == 2) step_env_t4(e, i, actions);
        else step_env(e, i, actions);
    }
}

/* ---------------------------------------------- Isaac-Gym tensor-API mode (TT:1022-1039) */
void ppo_post_physics_step(ppo_env* e, const float* rb_states /* [N,42,13] */, float* root_states /* [N,3,13] */,
                           float* dof_states /* [N,7,2] */, const float* dof_force /* [N,7] */,
                           const float* pre_ball_vx /* [N] */) {
    const ppenv_config* c = &e->cfg;
    static const int body_ids[NB] = {0, 31, 32, 33, 34, 35, 36, 37, 38, 39};
    for (int i = 0; i < e->n; i++) {
        const float* rb = &rb_states[(size_t)i * PPENV_NUM_BODIES * 13];
        float* root = &root_states[(size_t)i * PPENV_NUM_ACTORS * 13];
        float* dofs = &dof_states[(size_t)i * ND * 2];
        bodies_t bs;
        for (int j = 0; j < NB; j++) memcpy(bs[j], &rb[body_ids[j] * 13], 13 * sizeof(float));
        float qf[ND], qdf[ND];
        for (int d = 0; d < ND; d++) { qf[d] = dofs[2 * d]; qdf[d] = dofs[2 * d + 1]; }
        float* ball = &root[2 * 13];
        int64_t progress = e->progress[i] + 1;
        uint32_t flags = e->flags[i];
        int64_t reset;
        float rew = compute_reward(c, root[0], &rb[39 * 13], pre_ball_vx[i], ball, power_term(&dof_force[(size_t)i * ND], qdf, ND),
                                   progress, &flags, &reset);
        if (reset) {
            e->episode[i] += 1;
            float v[3];
            fresh_serve(e, i, v);
            const float* init_pos[3] = {c->humanoid_root_pos, c->table_root_pos, c->ball_init_pos};
            const float* init_quat[3] = {c->humanoid_root_quat, c->table_root_quat, c->ball_init_quat};
            for (int a = 0; a < 3; a++) {            /* TT:853-855 */
                memcpy(&root[a * 13], init_pos[a], 3 * sizeof(float));
                memcpy(&root[a * 13 + 3], init_quat[a], 4 * sizeof(float));
                memset(&root[a * 13 + 7], 0, 6 * sizeof(float));
            }
            memcpy(&ball[7], v, 3 * sizeof(float));  /* TT:857-862 */
            if (c->variant != PPENV_VARIANT_TN)
                for (int d = 0; d < ND; d++) { dofs[2 * d] = qf[d] = c->init_dof_pos[d]; dofs[2 * d + 1] = qdf[d] = c->init_dof_vel[d]; }
            progress = 0;
            flags = initial_flags(c);
        }
        e->progress[i] = progress; e->flags[i] = flags; e->rew[i] = rew; e->reset[i] = reset;
        compute_obs(bs, qf, qdf, ball, &e->obs[(size_t)i * PPENV_NUM_OBS]);
    }
}

/* ------------------------------------------------------------ refresh (gym.refresh_*)
 * 3-actor layouts [N,3,13] / [N,7,2] / [N,7] / [N,42,13]; 4-actor [N,4,13] (humanoid1, humanoid2, table, ball: T4:181-185) /
 * [N,14,2] / [N,14] / [N,82,13] (humanoid1 0-39, humanoid2 40-79, table 80, ball 81: T4:169-172). */
void ppo_refresh_root_states(ppo_env* e, float* out) {
    const ppenv_config* c = &e->cfg;
    const int A = e->A, rows = A + 2;
    for (int i = 0; i < e->n; i++) {
        float* r = &out[(size_t)i * rows * 13];
        memset(r, 0, rows * 13 * sizeof(float));
        memcpy(r, c->humanoid_root_pos, 12); memcpy(r + 3, c->humanoid_root_quat, 16);
        if (A == 2) { memcpy(r + 13, c->humanoid2_root_pos, 12); memcpy(r + 16, c->humanoid2_root_quat, 16); }
        memcpy(r + A * 13, c->table_root_pos, 12); memcpy(r + A * 13 + 3, c->table_root_quat, 16);
        for (int k = 0; k < 13; k++) r[(A + 1) * 13 + k] = e->ball[(size_t)k * e->n + i];
    }
}
void ppo_refresh_dof_states(ppo_env* e, float* out) {
    const int D = e->A * ND;
    for (int i = 0; i < e->n; i++)
        for (int d = 0; d < D; d++) {
            out[((size_t)i * D + d) * 2] = e->dof_pos[(size_t)d * e->n + i];
            out[((size_t)i * D + d) * 2 + 1] = e->dof_vel[(size_t)d * e->n + i];
        }
}
void ppo_refresh_dof_force(ppo_env* e, float* out) {
    const int D = e->A * ND;
    for (int i = 0; i < e->n; i++)
        for (int d = 0; d < D; d++) out[(size_t)i * D + d] = e->dof_force[(size_t)d * e->n + i];
}
void ppo_refresh_rigid_body_states(ppo_env* e, float* out) {
    const ppenv_config* c = &e->cfg;
    static const int body_ids[NB] = {0, 31, 32, 33, 34, 35, 36, 37, 38, 39};
    const int A = e->A, HB = PPENV_NUM_HUMANOID_BODIES;
    for (int i = 0; i < e->n; i++) {
        float qf[2 * ND], qdf[2 * ND], ball[13];
        gather_env(e, i, qf, qdf, ball);
        float* rb = &out[(size_t)i * (A * HB + 2) * 13];
        for (int a = 0; a < A; a++) {
            double q[ND], qd[ND];
            for (int d = 0; d < ND; d++) { q[d] = qf[a * ND + d]; qd[d] = qdf[a * ND + d]; }
            arm_fk k;
            arm_forward_kinematics_b(c, base_of(c, a), q, qd, &k);
            bodies_t bs;
            bodies_from_fk_arm(c, a, &k, bs);
            float* rba = &rb[a * HB * 13];
            const float* rp = a == 0 ? c->humanoid_root_pos : c->humanoid2_root_pos;
            const float* rq = a == 0 ? c->humanoid_root_quat : c->humanoid2_root_quat;
            for (int b = 0; b < HB; b++) {
                memset(&rba[b * 13], 0, 13 * sizeof(float));
                memcpy(&rba[b * 13], rp, 12); memcpy(&rba[b * 13 + 3], rq, 16);
            }
            for (int j = 0; j < NB; j++) memcpy(&rba[body_ids[j] * 13], bs[j], 13 * sizeof(float));
        }
        float* t = &rb[A * HB * 13];
        memset(t, 0, 13 * sizeof(float));
        memcpy(t, c->table_root_pos, 12); memcpy(t + 3, c->table_root_quat, 16);
        memcpy(t + 13, ball, 13 * sizeof(float));
    }
}

/* ---------------------------------------------------------------- state blob I/O */
size_t ppo_state_bytes(ppo_env* e) {
    size_t A = (size_t)e->A;
    return (size_t)e->n * ((A * ND * 3 + 13) * 4 + A * 4 + 4 + A * 8 + A * 8);
}
static unsigned char* blob_copy(unsigned char* p, void* arr, size_t bytes, int to_blob) {
    if (to_blob) memcpy(p, arr, bytes); else memcpy(arr, p, bytes);
    return p + bytes;
}
static void blob_io(ppo_env* e, unsigned char* p, int to_blob) {
    size_t n = e->n, A = (size_t)e->A;
    p = blob_copy(p, e->dof_pos, n * A * ND * 4, to_blob);
    p = blob_copy(p, e->dof_vel, n * A * ND * 4, to_blob);
    p = blob_copy(p, e->dof_force, n * A * ND * 4, to_blob);
    p = blob_copy(p, e->ball, n * 13 * 4, to_blob);
    p = blob_copy(p, e->flags, n * A * 4, to_blob);
    p = blob_copy(p, e->episode, n * 4, to_blob);
    p = blob_copy(p, e->progress, n * A * 8, to_blob);
    p = blob_copy(p, e->reset, n * A * 8, to_blob);
}
int ppo_get_state(ppo_env* e, void* dst, size_t nbytes) {
    if (nbytes != ppo_state_bytes(e)) return PPENV_ESTATE;
    blob_io(e, (unsigned char*)dst, 1);
    return 0;
}
int ppo_set_state(ppo_env* e, const void* src, size_t nbytes) {
    if (nbytes != ppo_state_bytes(e)) return PPENV_ESTATE;
    blob_io(e, (unsigned char*)src, 0);
    return 0;
}

/* ------------------------------------------------- exposed pieces for unit tests */
/* joint accelerations for one env (KAT: compare against the kernel's ABA) */
void ppo_arm_qdd(const ppenv_config* c, const double* q, const double* qd, const double* tau, const double* arm_eff,
                 double* qdd) {
    arm_fk k;
    arm_forward_kinematics(c, q, qd, &k);
    arm_forward_dynamics(c, &k, qd, tau, arm_eff, qdd);
}
void ppo_arm_inverse_dynamics(const ppenv_config* c, const double* q, const double* qd, const double* qdd, double* tau) {
    arm_fk k;
    arm_forward_kinematics(c, q, qd, &k);
    arm_rnea(c, &k, qd, qdd, -(double)c->gravity_z, 1, tau);
}
void ppo_arm_body_states(const ppenv_config* c, const double* q, const double* qd, float* out /* [10][13] */) {
    arm_fk k;
    arm_forward_kinematics(c, q, qd, &k);
    bodies_from_fk(c, &k, (float(*)[13])out);
}
/* total mechanical energy of the arm (kinetic + potential), for conservation tests */
double ppo_arm_energy(const ppenv_config* c, const double* q, const double* qd) {
    arm_fk k;
    arm_forward_kinematics(c, q, qd, &k);
    double E = 0;
    for (int i = 0; i < ND; i++) {
        const ppenv_joint* j = &c->joint[i];
        v3 comw = mv(&k.R[i], vf(j->com));
        v3 vc = vadd(k.v[i], vcross(k.w[i], comw));
        m3 I = {{j->inertia[0], j->inertia[3], j->inertia[4], j->inertia[3], j->inertia[1], j->inertia[5],
                 j->inertia[4], j->inertia[5], j->inertia[2]}};
        m3 Rt = mt(&k.R[i]);
        v3 wl = mv(&Rt, k.w[i]);
        E += 0.5 * j->mass * vdot(vc, vc) + 0.5 * vdot(wl, mv(&I, wl));
        E += -j->mass * c->gravity_z * (k.p[i].z + comw.z);
    }
    return E;
}
void ppo_serve_velocity(const ppenv_config* c, uint32_t gid, uint32_t episode, float out[3]) { serve_velocity(c, gid, episode, out); }
void ppo_serve_from_draws(int form, int m, const double* draws /* [m,3] */, float* out /* [m,3] */) {
    for (int i = 0; i < m; i++) serve_from_draws(form, draws[3 * i], draws[3 * i + 1], draws[3 * i + 2], &out[3 * i]);
}
void ppo_pd_targets(int m, int nd, const float* actions /* [m,nd] */, const float* lo, const float* hi /* [nd] */, float clip, float* out) {
    for (int i = 0; i < m; i++)
        for (int d = 0; d < nd; d++) out[(size_t)i * nd + d] = pd_target(actions[(size_t)i * nd + d], lo[d], hi[d], clip);
}
void ppo_compute_obs(const float* bodies /* [10][13] */, const float* dof_pos, const float* dof_vel, const float* ball, float* obs) {
    compute_obs((const float(*)[13])bodies, dof_pos, dof_vel, ball, obs);
}

/* ================================================================================================
 * 27-DoF variant, tensor-API mode: post_physics_step of tasks/humanoid_pingpong_3_actor_all_dof.py
 * ("TA") TA:1145-1192 on caller tensors.  fp32 in the reference's operation order.
 * ================================================================================================ */
#define TA_ND PPENV_TA_NUM_DOF
#define TA_NBAL PPENV_TA_NUM_BALANCE_BODIES
static const int ta_obs_ids[NB] = {0, 31, 32, 33, 34, 35, 36, 37, 38, 39};          /* bodyStatesIdPingpong, yaml:56 */
static const int ta_bal_ids[TA_NBAL] = {0, 2, 3, 4, 5, 6, 7, 9, 10, 11, 12, 13, 14, 15, 16, 17, 21, 22, 23, 24, 25, 26, 27}; /* yaml:57 */

/* compute_imitation_reward TA:1313-1418 with is_g1 = True */
static float ta_imitation_reward(const ppenv_ta_params* p, const float* rb, const float* irb, const float* dof_pos,
                                 const float* dof_vel, int* has_fallen) {
    const float k_pos = 50.f, k_vel = 4.0f, k_dof_pos = 5.0f, k_dof_vel = 0.05f;
    const float w_pos = 0.4f, w_vel = 0.2f, w_dof_pos = 0.2f, w_dof_vel = 0.2f;
    float pos_acc = 0.f, vel_acc = 0.f, norm_acc = 0.f;
    for (int j = 0; j < TA_NBAL; j++) {
        const float* b = &rb[ta_bal_ids[j] * 13];
        const float* r = &irb[ta_bal_ids[j] * 13];
        float dp0 = r[0] - b[0], dp1 = r[1] - b[1], dp2 = r[2] - b[2];
        float dv0 = r[7] - b[7], dv1 = r[8] - b[8], dv2 = r[9] - b[9];
        pos_acc += (dp0 * dp0 + dp1 * dp1 + dp2 * dp2) / 3.0f;      /* (diff**2).mean(-1) */
        vel_acc += (dv0 * dv0 + dv1 * dv1 + dv2 * dv2) / 3.0f;
        float e0 = b[0] - r[0], e1 = b[1] - r[1], e2 = b[2] - r[2];
        norm_acc += sqrtf(e0 * e0 + e1 * e1 + e2 * e2);             /* torch.norm(body_pos - ref_body_pos, dim=-1) */
    }
    float r_body_pos = expf(-k_pos * (pos_acc / (float)TA_NBAL));    /* TA:1349-1351 */
    float r_body_vel = expf(-k_vel * (vel_acc / (float)TA_NBAL));    /* TA:1354-1356 */
    float s22 = 0.f, s5 = 0.f, sv = 0.f;
    for (int d = 0; d < 22; d++) { float e = p->init_dof_pos[d] - dof_pos[d]; s22 += e * e; }
    for (int d = 22; d < TA_ND; d++) { float e = p->init_dof_pos[d] - dof_pos[d]; s5 += e * e; }
    for (int d = 0; d < 22; d++) { float e = p->init_dof_vel[d] - dof_vel[d]; sv += e * e; }
    float r22 = (w_dof_pos * 50.0f) * expf(-(k_dof_pos * 500.0f) * (s22 / 22.0f));   /* TA:1372-1380 */
    float r5 = w_dof_pos * expf(-k_dof_pos * (s5 / 5.0f));                             /* TA:1383-1387 */
    float r_dof_vel = expf(-k_dof_vel * (sv / 22.0f));                                 /* TA:1393,1401 */
    float ref = r22 + r5 + w_dof_vel * r_dof_vel + w_pos * r_body_pos + w_vel * r_body_vel;   /* TA:1403 */
    float term = p->is_train ? 0.32f : 1e6f;                                           /* TA:1407-1413 */
    *has_fallen = (norm_acc / (float)TA_NBAL) > term;                                  /* TA:1415 */
    if (*has_fallen) ref = 1.0f * -50.0f;                                              /* TA:1416-1417 */
    return ref;
}

void ppo_ta_post_physics_step(const ppenv_ta_params* p, const float* rb_states, const float* initial_rb_states,
                              float* root_states, float* dof_states, const float* dof_force, const float* pre_ball_vx,
                              const float* reset_override, uint32_t* flags, uint32_t* episode, int64_t* progress,
                              float* obs, float* rew, int64_t* reset_out) {
    const int n = p->num_envs;
    int any_reset = 0;
    for (int i = 0; i < n; i++) {
        const float* rb = &rb_states[(size_t)i * PPENV_NUM_BODIES * 13];
        const float* irb = &initial_rb_states[(size_t)(p->initial_rb_shared ? 0 : i) * PPENV_NUM_BODIES * 13];
        float* root = &root_states[(size_t)i * PPENV_NUM_ACTORS * 13];
        float* dofs = &dof_states[(size_t)i * TA_ND * 2];
        float* ball = &root[2 * 13];
        float q[TA_ND], qd[TA_ND];
        for (int d = 0; d < TA_ND; d++) { q[d] = dofs[2 * d]; qd[d] = dofs[2 * d + 1]; }
        int64_t prog = progress[i] + 1;                                      /* TA:1146 */
        uint32_t f = flags[i];
        const int paddle_cond = (f & PPENV_TA_FLAG_PADDLE_COND) != 0, hit_table_calc = (f & PPENV_TA_FLAG_HIT_TABLE_CALC) != 0;
        const int die_pen_calc = (f & PPENV_TA_FLAG_DIE_PENALTY_CALC) != 0, hum_die = (f & PPENV_TA_FLAG_HUMANOID_DIE_CALC) != 0;

        /* ---- compute_pingpong_reward_nv TA:1440-1690 */
        const float* paddle = &rb[39 * 13];
        const float bx = ball[0], by = ball[1], bz = ball[2], vx = ball[7], pvx = pre_ball_vx[i];
        int has_fallen;
        float ref_reward = ta_imitation_reward(p, rb, irb, q, qd, &has_fallen);   /* TA:1492 */
        float pelvis_h = rb[2];                                                   /* humanoid1_pelvis_rb_states[..., 2] */
        if (has_fallen) f |= PPENV_TA_COUNT_FALL_DOWN;                            /* TA:1525-1529 */
        int x_close = fabsf(bx - paddle[0]) < 0.2f;                               /* TA:1544 */
        int first_close = x_close && !paddle_cond;                                /* TA:1545 */
        float dy = by - paddle[1], dz = bz - paddle[2];
        float yz = sqrtf(dy * dy + dz * dz);                                      /* TA:1548 */
        int in_circle = yz < 0.15f;
        float pos_reward = 0.f;
        if (first_close && !hum_die) pos_reward = in_circle ? p->hit_paddle_reward : p->miss_paddle_penalty_coefficient * yz;   /* TA:1555-1563 */
        if (first_close && in_circle) f |= PPENV_TA_COUNT_CLOSER;                 /* TA:1566-1570 */
        int hit_paddle = pvx < 0.f && vx > 1.5f;                                  /* TA:1577 */
        if (hit_paddle) f |= PPENV_TA_COUNT_HIT_PADDLE;                           /* TA:1579-1583 */
        float vel_reward = (hit_paddle && !paddle_cond && !hum_die) ? p->alpha_velocity_reward * fabsf(vx) : 0.f;   /* TA:1586-1590 */
        if (x_close) f |= PPENV_TA_FLAG_PADDLE_COND;                              /* TA:1595 */
        float humanoid_x = root[0];
        float time_penalty = (bx > humanoid_x && vx < 0.f) ? -0.01f * (float)prog : 0.f;   /* TA:1602-1607 */
        /* compute_gradient_penalty TA:1245-1301 */
        int z_in = bz >= 0.82f && bz <= 0.83f && vx > 0.f;
        float ddx = bx - 2.5f, ddy = by - 0.0f;
        float dist = sqrtf(ddx * ddx + ddy * ddy);
        int in_range = bx >= 1.9f && bx <= 3.1f && by >= -0.6f && by <= 0.6f;
        if (z_in && in_range) f |= PPENV_TA_COUNT_HIT_TABLE;
        float hit_rp = 0.f;
        if (z_in && !hit_table_calc && !hum_die) hit_rp = in_range ? p->hit_table_reward : p->not_hit_table_penalty * dist;
        if (z_in) f |= PPENV_TA_FLAG_HIT_TABLE_CALC;
        /* net TA:1619-1650 */
        int over_net = bx > 1.72f && bx < 1.78f && vx > 0.f;
        int suitable = bz > 0.96f && bz < 1.25f;
        float over_h = 0.f;
        if (!suitable) over_h = bz > 1.25f ? bz - 1.25f : 0.96f - bz;
        float net_rp = 0.f;
        if (over_net && !hum_die) net_rp = suitable ? p->cross_net_reward : -400.f * over_h;
        if (net_rp > 0.f) f |= PPENV_TA_COUNT_CROSS_NET;                          /* TA:1652-1656 */
        float power = 0.f;
        for (int d = 0; d < TA_ND; d++) power += fabsf(dof_force[(size_t)i * TA_ND + d] * qd[d]);
        float power_reward = -p->power_coefficient * power;                       /* TA:1664-1665 */
        float die_penalty = (bz < 0.78f && !die_pen_calc && !hum_die) ? p->die_penalty : 0.f;   /* TA:1677-1679 */
        if (bz < 0.78f) f |= PPENV_TA_FLAG_DIE_PENALTY_CALC;                      /* TA:1681 */
        if (pelvis_h < 0.97f) f |= PPENV_TA_FLAG_HUMANOID_DIE_CALC;               /* TA:1683 */
        float reward = 0.f + (((((((pos_reward + power_reward) + vel_reward) + hit_rp) + net_rp) + die_penalty) + time_penalty) + ref_reward);   /* TA:1686 */
        int64_t rst = (prog >= (int64_t)p->max_episode_length - 1) ? 1 : 0;       /* TA:1688: time-out only */

        /* ---- _reset_idx TA:965-1028 */
        if (rst) {
            any_reset = 1;
            episode[i] += 1;
            float ov[5];
            if (reset_override) memcpy(ov, &reset_override[(size_t)i * 5], sizeof ov);
            else {
                uint32_t gid = (uint32_t)(p->env_id_offset + i), ep = episode[i];
                float u[5];
                for (int k = 0; k < 5; k++) {
                    uint64_t s = mix64(p->seed + 0x9E3779B97F4A7C15ull * ((uint64_t)gid + 1));
                    uint64_t x = mix64(s + 0x9E3779B97F4A7C15ull * ((uint64_t)ep * 8 + k + 1));
                    u[k] = (float)(x >> 40) * (1.0f / 16777216.0f);
                }
                ov[0] = p->ball_y_lo + (p->ball_y_hi - p->ball_y_lo) * u[0];      /* draw order TA:976-979: y, z, speed, tilt, tilt_z */
                ov[1] = p->ball_z_lo + (p->ball_z_hi - p->ball_z_lo) * u[1];
                double speed = p->serve_speed_lo + (p->serve_speed_hi - p->serve_speed_lo) * u[2];
                double a = p->serve_tilt_lo_deg + (p->serve_tilt_hi_deg - p->serve_tilt_lo_deg) * u[3];
                double az = p->serve_tilt_z_lo_deg + (p->serve_tilt_z_hi_deg - p->serve_tilt_z_lo_deg) * u[4];
                serve_from_draws(PPENV_VARIANT_TN, speed, a, az, &ov[2]);          /* TA:370-375 is TN's form */
            }
            for (int a = 0; a < 3; a++) {
                memcpy(&root[a * 13], p->init_root[a], 7 * sizeof(float));
                memset(&root[a * 13 + 7], 0, 6 * sizeof(float));
            }
            ball[1] = ov[0]; ball[2] = ov[1]; ball[7] = ov[2]; ball[8] = ov[3]; ball[9] = ov[4];
            for (int d = 0; d < TA_ND; d++) { dofs[2 * d] = q[d] = p->init_dof_pos[d]; dofs[2 * d + 1] = qd[d] = p->init_dof_vel[d]; }
            prog = 0;
            f &= ~(PPENV_TA_FLAG_PADDLE_COND | PPENV_TA_FLAG_DIE_PENALTY_CALC | PPENV_TA_FLAG_HUMANOID_DIE_CALC | PPENV_TA_FLAG_HIT_TABLE_CALC);   /* TA:1021-1024 */
        }
        progress[i] = prog; flags[i] = f; rew[i] = reward; reset_out[i] = rst;

        /* ---- compute_observations TA:867-904 (body states pre-reset, dof / ball post-reset) */
        float* o = &obs[(size_t)i * PPENV_TA_NUM_OBS];
        float hinv[4];
        heading_quat_inv_f(&rb[3], hinv);
        const float* rootp = &rb[0];
        for (int j = 0; j < NB; j++) {
            const float* b = &rb[ta_obs_ids[j] * 13];
            float rel[3] = {b[0] - rootp[0], b[1] - rootp[1], b[2] - rootp[2]};
            quat_rotate_f(hinv, rel, &o[3 * j]);
            quat_rotate_f(hinv, &b[7], &o[30 + 3 * j]);
        }
        for (int d = 0; d < TA_ND; d++) { o[60 + d] = q[d]; o[60 + TA_ND + d] = qd[d] * 0.1f; }
        float lb[3], lv[3];
        float relb[3] = {ball[0] - rootp[0], ball[1] - rootp[1], ball[2] - rootp[2]};
        quat_rotate_f(hinv, relb, lb);
        quat_rotate_f(hinv, &ball[7], lv);
        o[114] = lb[0]; o[115] = lb[1]; o[116] = lb[2]; o[117] = lv[0]; o[118] = lv[1]; o[119] = lv[2];
        o[120] = lb[1] + (lv[1] / (-lv[0] + 1e-6f)) * lb[0];                       /* TA:1839 */
        for (int j = 0; j < TA_NBAL; j++) {                                        /* TA:1891-1927 */
            const float* b = &rb[ta_bal_ids[j] * 13];
            const float* r = &irb[ta_bal_ids[j] * 13];
            float dp[3] = {r[0] - b[0], r[1] - b[1], r[2] - b[2]}, dv[3] = {r[7] - b[7], r[8] - b[8], r[9] - b[9]}, t[3];
            quat_rotate_f(hinv, dp, t);
            o[121 + 3 * j] = t[0] * 10.f; o[122 + 3 * j] = t[1] * 10.f; o[123 + 3 * j] = t[2] * 10.f;
            quat_rotate_f(hinv, dv, &o[121 + 3 * TA_NBAL + 3 * j]);
        }
        for (int d = 0; d < TA_ND; d++) { o[121 + 6 * TA_NBAL + d] = p->init_dof_pos[d]; o[121 + 6 * TA_NBAL + TA_ND + d] = p->init_dof_vel[d]; }
    }
    if (any_reset)                                                                  /* TA:1162-1166: fill_(0) on ALL envs */
        for (int i = 0; i < n; i++) flags[i] &= ~PPENV_TA_COUNT_MASK;
}

/* ================================================================================================
 * 4-actor variant: the two reward functions of tasks/humanoid_pingpong_4_actor_tilt.py (T4:1113-1439).
 * ================================================================================================ */

/* compute_humanoid2_pingpong_reward T4:1280-1439: TT's reward mirrored for the humanoid at the far end */
static float t4_reward_side2(const ppenv_t4_params* p, float humanoid_x, const float* paddle, float pre_vx, const float* ball,
                             float power, int64_t progress, uint32_t* flags, int64_t* reset_out) {
    const float Bx = ball[0], By = ball[1], Bz = ball[2], vx = ball[7];
    uint32_t f = *flags;
    float dx = paddle[0] - Bx, dy = paddle[1] - By, dz = paddle[2] - Bz;
    float dist = sqrtf(dx * dx + dy * dy + dz * dz);
    float pos_reward = 1.0f / (1.0f + 1.5f * dist * dist);                                   /* T4:1305-1308 */
    int cond = pre_vx > 0.0f && vx < 0.0f;                                                   /* T4:1328 */
    float vel_reward = (cond && !(f & PPENV_FLAG_COND_CALC)) ? p->alpha_velocity_reward * fabsf(vx) : 0.0f;
    if (cond) f |= PPENV_FLAG_COND_CALC;
    int missed = Bx > humanoid_x + 0.05f;                                                    /* T4:1344 */
    float reward = missed ? 0.0f + p->penalty : 0.0f;
    int bounce = Bz < 0.83f && vx < 0.0f && By < 0.6f && By > -0.6f;                         /* T4:1359 */
    float hit = 0.0f;
    int early = Bx > 1.06f && bounce;                                                        /* T4:1363 */
    if (early && !(f & PPENV_FLAG_REWARD_CALC)) hit = p->not_hit_table_penalty;
    if (early) { f |= PPENV_FLAG_REWARD_CALC; f &= ~PPENV_FLAG_NO_BOUNCE; }
    int inx = Bx < 1.06f && Bx > 0.4f;                                                       /* T4:1374 */
    int good = inx && bounce && (f & PPENV_FLAG_NO_BOUNCE);
    if (good && !(f & PPENV_FLAG_REWARD_CALC)) hit = p->hit_table_reward;
    if (good) f |= PPENV_FLAG_REWARD_CALC;
    if (Bx <= 0.4f && vx < 0.0f && !(f & PPENV_FLAG_REWARD_CALC)) hit = p->not_hit_table_penalty;   /* T4:1384 */
    if (Bx <= 0.4f) f |= PPENV_FLAG_REWARD_CALC;                                             /* T4:1389 */
    float net = (Bx > 1.7f && Bx < 1.8f && vx < 0.0f && By < 0.4f && By > -0.4f && Bz > 0.98f && Bz < 1.14f) ? 400.0f : 0.0f;   /* T4:1401-1409 */
    float power_reward = -p->power_coefficient * power;
    reward += (((pos_reward + power_reward) + vel_reward) + hit) + net;                      /* T4:1426 */
    int64_t die = Bz < 0.1f ? 1 : 0;
    *flags = f;
    *reset_out = (progress >= (int64_t)p->max_episode_length - 1) ? 1 : die;
    return reward;
}

void ppo_t4_rewards(const ppenv_t4_params* p, const float* rb_states, const float* root_states, const float* dof_states,
                    const float* dof_force, const float* pre_ball_vx, const int64_t* progress, const uint32_t* flags1_in,
                    const uint32_t* flags2_in, uint32_t* flags1, uint32_t* flags2, float* rew1, float* rew2, int64_t* reset1,
                    int64_t* reset2) {
    ppenv_config c;   /* side 1 is TT's function verbatim (T4:1113-1278 == TT:1105-1270): reuse its restatement */
    memset(&c, 0, sizeof c);
    c.variant = PPENV_VARIANT_TT;
    c.max_episode_length = p->max_episode_length;
    c.alpha_velocity_reward = p->alpha_velocity_reward; c.power_coefficient = p->power_coefficient; c.penalty = p->penalty;
    c.hit_table_reward = p->hit_table_reward; c.not_hit_table_penalty = p->not_hit_table_penalty;
    for (int i = 0; i < p->num_envs; i++) {
        const float* rb = &rb_states[(size_t)i * PPENV_T4_NUM_BODIES * 13];
        const float* root = &root_states[(size_t)i * PPENV_T4_NUM_ACTORS * 13];
        const float* ball = &root[3 * 13];
        float power = 0.f;
        for (int d = 0; d < PPENV_T4_NUM_DOF; d++)       /* the class hands the whole 14-dof tensors to the reward (T4:746-747) */
            power += fabsf(dof_force[(size_t)i * PPENV_T4_NUM_DOF + d] * dof_states[((size_t)i * PPENV_T4_NUM_DOF + d) * 2 + 1]);
        flags1[i] = flags1_in[i]; flags2[i] = flags2_in[i];
        rew1[i] = compute_reward(&c, root[0], &rb[39 * 13], pre_ball_vx[i], ball, power, progress[i], &flags1[i], &reset1[i]);
        rew2[i] = t4_reward_side2(p, root[13], &rb[79 * 13], pre_ball_vx[i], ball, power, progress[i], &flags2[i], &reset2[i]);
    }
}

/* ------------------------------------------------ the fused step of the 4-actor variant (PPENV_VARIANT_T4)
 * Two humanoids (the same arm model on two bases), one ball.  Reference pieces: pre_physics_step T4:1008-1026, the two
 * reward functions T4:1113-1439, _reset_idx T4:853-912 (both humanoids' dof states, all four actors' root states),
 * observations per humanoid T4:770-803.  The class itself is unfinished (T4:743 calls a missing name, T4:786 "TODO");
 * the wiring — agent a of env e owns row 2e + a, each agent observes its own seven dofs, one shared reset — is the
 * build's completion (include/ppenv.h, PPENV_VARIANT_T4).  Like the class's call site (T4:746-747), both reward
 * functions receive the whole 14-dof force / velocity tensors. */
static void step_env_t4(ppo_env* e, int i, const float* actions) {
    const ppenv_config* c = e->cfg_env ? &e->cfg_env[i] : &e->cfg;      /* domain randomisation: this env's own scaled model (both humanoids) */
    const int n = e->n;
    float qf[2 * ND], qdf[2 * ND], ballf[13];
    gather_env(e, i, qf, qdf, ballf);
    const uint32_t dr_gid = (uint32_t)(c->env_id_offset + i), dr_ep = e->episode[i], dr_prog = (uint32_t)e->progress[(size_t)i * 2];

    double target[2][ND], q[2][ND], qd[2][ND], tau_drive[2][ND] = {{0}};
    for (int a = 0; a < 2; a++)
        for (int d = 0; d < ND; d++) {
            float act = actions[((size_t)i * 2 + a) * ND + d];
            if (e->dr_action_sigma > 0.f) act += e->dr_action_sigma * dr_gauss(c->seed, dr_gid, dr_ep, dr_prog, (uint32_t)(a * ND + d));   /* indices 0 .. 13 */
            target[a][d] = pd_target(act, c->joint[d].lower, c->joint[d].upper, c->clip_actions);   /* T4:1014 */
            q[a][d] = qf[a * ND + d]; qd[a][d] = qdf[a * ND + d];
        }
    float pre_vx = ballf[7];                                        /* T4:1026 */

    ball_t b = {vf(&ballf[0]), vf(&ballf[7]), vf(&ballf[10])};
    double bq[4] = {ballf[3], ballf[4], ballf[5], ballf[6]};
    double h = (double)c->dt / c->substeps;
    arm_fk k0[2];
    for (int a = 0; a < 2; a++) arm_forward_kinematics_b(c, base_of(c, a), q[a], qd[a], &k0[a]);
    for (int s = 0; s < c->substeps; s++) {
        arm_geom g[2];
        for (int a = 0; a < 2; a++) {
            double tau[ND], arm_eff[ND], qdd[ND];
            arm_geometry_s(c, a == 0 ? c->shape : c->shape2, &k0[a], &g[a]);   /* pose and velocities at the start of the substep */
            for (int d = 0; d < ND; d++) {
                const ppenv_joint* j = &c->joint[d];
                double err = target[a][d] - q[a][d];
                tau[d] = clampd(j->kp * (err - h * qd[a][d]) - j->kd * qd[a][d], -j->effort, j->effort);
                arm_eff[d] = j->armature + h * j->kd + h * h * j->kp;
            }
            arm_forward_dynamics_b(c, base_of(c, a), &k0[a], qd[a], tau, arm_eff, qdd);
            for (int d = 0; d < ND; d++) {
                const ppenv_joint* j = &c->joint[d];
                double err = target[a][d] - q[a][d];
                double v_new = qd[a][d] + h * qdd[d];
                tau_drive[a][d] = clampd(j->kp * (err - h * v_new) - j->kd * v_new, -j->effort, j->effort);
                v_new = clampd(v_new, -j->vel_limit, j->vel_limit);
                double q_new = q[a][d] + h * v_new;
                if (q_new > j->upper) { q_new = j->upper; if (v_new > 0) v_new = 0; }
                if (q_new < j->lower) { q_new = j->lower; if (v_new < 0) v_new = 0; }
                q[a][d] = q_new; qd[a][d] = v_new;
            }
        }
        const arm_geom* garr[2] = {&g[0], &g[1]};
        ball_substep_n(c, &b, bq, 2, garr, h);
        for (int a = 0; a < 2; a++) arm_forward_kinematics_b(c, base_of(c, a), q[a], qd[a], &k0[a]);
    }

    /* refresh_sim_tensors: round the state to the fp32 tensors */
    float dof_force[2 * ND];
    for (int a = 0; a < 2; a++)
        for (int d = 0; d < ND; d++) {
            qf[a * ND + d] = (float)q[a][d]; qdf[a * ND + d] = (float)qd[a][d]; dof_force[a * ND + d] = (float)tau_drive[a][d];
        }
    ballf[0] = (float)b.p.x; ballf[1] = (float)b.p.y; ballf[2] = (float)b.p.z;
    for (int t = 0; t < 4; t++) ballf[3 + t] = (float)bq[t];
    ballf[7] = (float)b.v.x; ballf[8] = (float)b.v.y; ballf[9] = (float)b.v.z;
    ballf[10] = (float)b.w.x; ballf[11] = (float)b.w.y; ballf[12] = (float)b.w.z;
    bodies_t bs[2];
    for (int a = 0; a < 2; a++) bodies_from_fk_arm(c, a, &k0[a], bs[a]);

    /* post_physics_step: T4:1028-1046 */
    int64_t progress = e->progress[(size_t)i * 2] + 1;
    uint32_t flags[2] = {e->flags[i], e->flags[(size_t)n + i]};
    int64_t reset1, reset2;
    float power = power_term(dof_force, qdf, 2 * ND);               /* T4:746-747: the whole dof tensors */
    ppenv_t4_params p;
    memset(&p, 0, sizeof p);
    p.max_episode_length = c->max_episode_length;
    p.alpha_velocity_reward = c->alpha_velocity_reward; p.power_coefficient = c->power_coefficient; p.penalty = c->penalty;
    p.hit_table_reward = c->hit_table_reward; p.not_hit_table_penalty = c->not_hit_table_penalty;
    float rew1 = compute_reward(c, c->humanoid_root_pos[0], bs[0][c->paddle_obs_index], pre_vx, ballf, power, progress, &flags[0], &reset1);
    float rew2 = t4_reward_side2(&p, c->humanoid2_root_pos[0], bs[1][c->paddle_obs_index], pre_vx, ballf, power, progress, &flags[1], &reset2);
    int64_t reset = (reset1 | reset2) ? 1 : 0;                      /* same rule on both sides (T4:1270-1276, 1431-1437) */
    for (int d = 0; d < 2 * ND; d++) {
        e->dof_pos[(size_t)d * n + i] = qf[d]; e->dof_vel[(size_t)d * n + i] = qdf[d]; e->dof_force[(size_t)d * n + i] = dof_force[d];
    }
    for (int t = 0; t < 13; t++) e->ball[(size_t)t * n + i] = ballf[t];
    if (reset) {                                                    /* T4:853-912 */
        e->episode[i] += 1;
        reset_env_state(e, i, 1);
        progress = 0;
        flags[0] = flags[1] = initial_flags(c);
        gather_env(e, i, qf, qdf, ballf);
    }
    for (int a = 0; a < 2; a++) {
        e->progress[(size_t)i * 2 + a] = progress; e->flags[(size_t)a * n + i] = flags[a]; e->reset[(size_t)i * 2 + a] = reset;
        compute_obs(bs[a], &qf[a * ND], &qdf[a * ND], ballf, &e->obs[((size_t)i * 2 + a) * PPENV_NUM_OBS]);
        if (e->dr_obs_sigma > 0.f)       /* agent a's row: indices 16 + 80 a + k (clear of the 14 action draws, < 256) */
            for (int k = 0; k < PPENV_NUM_OBS; k++)
                e->obs[((size_t)i * 2 + a) * PPENV_NUM_OBS + k] += e->dr_obs_sigma * dr_gauss(c->seed, dr_gid, dr_ep, dr_prog, 16u + (uint32_t)(a * PPENV_NUM_OBS + k));
    }
    e->rew[(size_t)i * 2] = rew1; e->rew[(size_t)i * 2 + 1] = rew2;
}

/* ================================================================================================
 * 27-DoF variant: the rigid-body step (ppenv_ta_simulate).  PARITY UNPINNED (Isaac Gym / PhysX is closed and absent, the
 * g1_27dof.urdf asset TA:470 too): this restates the build's own specification, DESIGN.md "TA physics":
 *   - free-floating 28-link tree, generalised velocity nu = [omega_b, v_b (base twist, base coordinates), qd]
 *   - gravity as a force; PD drives as for the arm (explicit test against the effort limit, else implicit)
 *   - feet: penalty contacts at the sole corners, active while penetrating and pushing; normal spring-damper and, while
 *     tangential damper (coefficient capped at mu f_n / |v_t|: Coulomb) integrated implicitly: f(v+) ~ f(v) - h D a with a
 *     the link's spatial acceleration, i.e. h J^T D J is added to the link's inertia in the inertia term
 *   - semi-implicit Euler; the base in world coordinates (classical acceleration R (a + omega x v))
 *   - the ball against the humanoid's shapes exactly as in the 3-actor scenes (start-of-substep geometry)
 * Algorithm here: inertia matrix and bias by recursive Newton-Euler sweeps + dense 33x33 solve in fp64 (the kernel runs the
 * floating-base articulated-body algorithm in fp32).
 * ================================================================================================ */
#define TL PPENV_TA_NUM_LINKS
#define TNV (6 + PPENV_TA_NUM_DOF)
typedef struct { double a[6]; } sv6;                 /* spatial vector, angular part first, link coordinates */
typedef struct { double m[6][6]; } sm6;
typedef struct {
    m3 E[TL];          /* child -> parent rotation */
    v3 r[TL];          /* child origin in the parent frame */
    m3 Rw[TL]; v3 pw[TL];
    sv6 v[TL];         /* link twist, link coordinates */
    sv6 c[TL];         /* velocity-product acceleration v x S qd */
} ta_kin;

static sv6 sv_zero(void) { sv6 z; memset(&z, 0, sizeof z); return z; }
static v3 sv_ang(const sv6* s) { return V(s->a[0], s->a[1], s->a[2]); }
static v3 sv_lin(const sv6* s) { return V(s->a[3], s->a[4], s->a[5]); }
static sv6 sv_make(v3 a, v3 l) { sv6 s = {{a.x, a.y, a.z, l.x, l.y, l.z}}; return s; }
/* motion vector parent -> child coordinates */
static sv6 xm(const m3* E, v3 r, const sv6* vp) {
    m3 Et = mt(E);
    v3 w = sv_ang(vp), l = sv_lin(vp);
    return sv_make(mv(&Et, w), mv(&Et, vadd(l, vcross(w, r))));
}
/* force vector child -> parent coordinates */
static sv6 xf(const m3* E, v3 r, const sv6* fc) {
    v3 n = mv(E, sv_ang(fc)), f = mv(E, sv_lin(fc));
    return sv_make(vadd(n, vcross(r, f)), f);
}
static sm6 spatial_inertia(double mass, const float* com, const float* in6) {
    sm6 I; memset(&I, 0, sizeof I);
    double c[3] = {com[0], com[1], com[2]};
    double Ic[3][3] = {{in6[0], in6[3], in6[4]}, {in6[3], in6[1], in6[5]}, {in6[4], in6[5], in6[2]}};
    double cx[3][3] = {{0, -c[2], c[1]}, {c[2], 0, -c[0]}, {-c[1], c[0], 0}};
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            double cc = 0;
            for (int k = 0; k < 3; k++) cc += cx[i][k] * cx[j][k];           /* c^ c^T */
            I.m[i][j] = Ic[i][j] + mass * cc;
            I.m[i][3 + j] = mass * cx[i][j];
            I.m[3 + i][j] = mass * cx[j][i];
        }
    for (int i = 0; i < 3; i++) I.m[3 + i][3 + i] = mass;
    return I;
}
static sv6 sm_mul(const sm6* I, const sv6* v) {
    sv6 r;
    for (int i = 0; i < 6; i++) { double s = 0; for (int j = 0; j < 6; j++) s += I->m[i][j] * v->a[j]; r.a[i] = s; }
    return r;
}
/* v x* f */
static sv6 crf(const sv6* v, const sv6* f) {
    v3 w = sv_ang(v), l = sv_lin(v), n = sv_ang(f), ff = sv_lin(f);
    return sv_make(vadd(vcross(w, n), vcross(l, ff)), vcross(w, ff));
}
/* v x m */
static sv6 crm(const sv6* v, const sv6* m) {
    v3 w = sv_ang(v), l = sv_lin(v), mw = sv_ang(m), ml = sv_lin(m);
    return sv_make(vcross(w, mw), vadd(vcross(w, ml), vcross(l, mw)));
}

/* base: position, xyzw quaternion, linear and angular velocity in world coordinates (the root_states row layout) */
static void ta_kinematics_d(const ppenv_ta_model* M, const double* pos, const double* quat, const double* vw, const double* ww,
                            const double* q, const double* qd, ta_kin* k) {
    double x = quat[0], y = quat[1], z = quat[2], w = quat[3];
    m3 R0 = {{1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z),
              2 * (y * z - x * w), 2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)}};
    m3 R0t = mt(&R0);
    k->Rw[0] = R0; k->pw[0] = V(pos[0], pos[1], pos[2]);
    k->v[0] = sv_make(mv(&R0t, V(ww[0], ww[1], ww[2])), mv(&R0t, V(vw[0], vw[1], vw[2])));
    k->c[0] = sv_zero();
    for (int i = 1; i < TL; i++) {
        const ppenv_ta_link* L = &M->link[i];
        int p = L->parent;
        m3 R0j = mf(L->origin_rot), Rq = axis_rot(L->axis, q[i - 1]);
        k->E[i] = mm(&R0j, &Rq);
        k->r[i] = vf(L->origin_xyz);
        k->Rw[i] = mm(&k->Rw[p], &k->E[i]);
        k->pw[i] = vadd(k->pw[p], mv(&k->Rw[p], k->r[i]));
        sv6 vj = sv_zero();
        vj.a[L->axis] = qd[i - 1];
        sv6 vp = xm(&k->E[i], k->r[i], &k->v[p]);
        for (int t = 0; t < 6; t++) k->v[i].a[t] = vp.a[t] + vj.a[t];
        k->c[i] = crm(&k->v[i], &vj);
    }
}
static void ta_kinematics(const ppenv_ta_model* M, const float* root /*13*/, const double* q, const double* qd, ta_kin* k) {
    double pos[3] = {root[0], root[1], root[2]}, quat[4] = {root[3], root[4], root[5], root[6]};
    double vw[3] = {root[7], root[8], root[9]}, ww[3] = {root[10], root[11], root[12]};
    ta_kinematics_d(M, pos, quat, vw, ww, q, qd, k);
}

/* Recursive Newton-Euler over the tree.  a0: base spatial acceleration; qdd [27].  The inertia term uses I + dI (implicit
 * contact dampers); use_vel adds the velocity products and -fext.  Returns the base force and the joint torques. */
static void ta_rnea(const ppenv_ta_model* M, const ta_kin* k, const sm6* I, const sm6* dI, const sv6* fext, const sv6* a0,
                    const double* qdd, int use_vel, sv6* f0, double* tau) {
    sv6 a[TL], f[TL];
    a[0] = *a0;
    for (int i = 0; i < TL; i++) {
        if (i > 0) {
            const ppenv_ta_link* L = &M->link[i];
            a[i] = xm(&k->E[i], k->r[i], &a[L->parent]);
            a[i].a[L->axis] += qdd[i - 1];
            if (use_vel) for (int t = 0; t < 6; t++) a[i].a[t] += k->c[i].a[t];
        }
        sm6 It = I[i];
        for (int r = 0; r < 6; r++) for (int cidx = 0; cidx < 6; cidx++) It.m[r][cidx] += dI[i].m[r][cidx];
        f[i] = sm_mul(&It, &a[i]);
        if (use_vel) {
            sv6 h = sm_mul(&I[i], &k->v[i]);
            sv6 b = crf(&k->v[i], &h);
            for (int t = 0; t < 6; t++) f[i].a[t] += b.a[t] - fext[i].a[t];
        }
    }
    for (int i = TL - 1; i >= 1; i--) {
        const ppenv_ta_link* L = &M->link[i];
        tau[i - 1] = f[i].a[L->axis];
        sv6 fp = xf(&k->E[i], k->r[i], &f[i]);
        for (int t = 0; t < 6; t++) f[L->parent].a[t] += fp.a[t];
    }
    *f0 = f[0];
}

static int solve_dense(int n, double* A /* n x n row-major */, double* b) {
    for (int col = 0; col < n; col++) {
        int piv = col;
        for (int r = col + 1; r < n; r++) if (fabs(A[r * n + col]) > fabs(A[piv * n + col])) piv = r;
        if (fabs(A[piv * n + col]) < 1e-300) return -1;
        if (piv != col) {
            for (int cidx = 0; cidx < n; cidx++) { double t = A[col * n + cidx]; A[col * n + cidx] = A[piv * n + cidx]; A[piv * n + cidx] = t; }
            double t = b[col]; b[col] = b[piv]; b[piv] = t;
        }
        for (int r = col + 1; r < n; r++) {
            double f = A[r * n + col] / A[col * n + col];
            if (f == 0) continue;
            for (int cidx = col; cidx < n; cidx++) A[r * n + cidx] -= f * A[col * n + cidx];
            b[r] -= f * b[col];
        }
    }
    for (int r = n - 1; r >= 0; r--) {
        double sum = b[r];
        for (int cidx = r + 1; cidx < n; cidx++) sum -= A[r * n + cidx] * b[cidx];
        b[r] = sum / A[r * n + r];
    }
    return 0;
}

/* external force on each link (gravity + foot contacts) and the implicit contact dampers dI = h J^T D J */
static void ta_external(const ppenv_config* c, const ppenv_ta_model* M, const ta_kin* k, double h, sv6* fext, sm6* dI) {
    for (int i = 0; i < TL; i++) {
        const ppenv_ta_link* L = &M->link[i];
        m3 Rt = mt(&k->Rw[i]);
        v3 fg = mv(&Rt, V(0, 0, L->mass * (double)c->gravity_z));
        fext[i] = sv_make(vcross(vf(L->com), fg), fg);
        memset(&dI[i], 0, sizeof(sm6));
    }
    for (int cp = 0; cp < M->num_contacts; cp++) {
        int li = M->contact_link[cp];
        m3 R = k->Rw[li], Rt = mt(&R);
        v3 w = sv_ang(&k->v[li]), vl = sv_lin(&k->v[li]);
        {
            v3 r = vf(M->contact_point[cp]);
            v3 pw = vadd(k->pw[li], mv(&R, r));
            double pen = (double)M->ground_z - pw.z;
            if (!(pen > 0)) continue;
            v3 vw = mv(&R, vadd(vl, vcross(w, r)));
            /* Every switch of the contact law is a ramp, so that a state within rounding of one does not change the step:
             * the damper's coefficient grows with the overlap up to contact_fade_depth (Hunt-Crossley-like; the ramp must
             * not be steep: it acts as an extra stiffness c_n v_z / fade_depth), the implicit terms fade in with the force. */
            double wfade = pen < (double)M->contact_fade_depth ? pen / (double)M->contact_fade_depth : 1.0;
            double pc = pen > (double)M->contact_max_penetration ? (double)M->contact_max_penetration : pen;   /* saturating spring */
            double fn0 = M->foot_stiffness * pc - wfade * M->foot_damping * vw.z;
            if (!(fn0 > 0)) continue;
            double gfade = fn0 < (double)M->contact_fade_force ? fn0 / (double)M->contact_fade_force : 1.0;
            /* friction: a tangential damper whose coefficient is capped so that its force never exceeds mu f_n (the secant
             * of Coulomb's law at the current slip speed); implicit in either regime, so it cannot reverse the slip */
            double vt = sqrt(vw.x * vw.x + vw.y * vw.y);
            double dt_imp = gfade * M->foot_tangent_damping;
            if (dt_imp * vt > M->foot_friction * fn0) dt_imp = M->foot_friction * fn0 / vt;
            v3 fw = V(-dt_imp * vw.x, -dt_imp * vw.y, fn0);
            v3 fb = mv(&Rt, fw);
            sv6 add = sv_make(vcross(r, fb), fb);
            for (int t = 0; t < 6; t++) fext[li].a[t] += add.a[t];
            /* D_b = R^T diag(dt, dt, cn + h k) R; J = [-r^, 1] */
            double dw[3] = {dt_imp, dt_imp, gfade * (wfade * M->foot_damping + h * M->foot_stiffness)};
            double Db[3][3];
            for (int a = 0; a < 3; a++)
                for (int b2 = 0; b2 < 3; b2++) {
                    double sum = 0;
                    for (int t = 0; t < 3; t++) sum += R.m[3 * t + a] * dw[t] * R.m[3 * t + b2];
                    Db[a][b2] = sum;
                }
            double J[3][6] = {{0, r.z, -r.y, 1, 0, 0}, {-r.z, 0, r.x, 0, 1, 0}, {r.y, -r.x, 0, 0, 0, 1}};
            for (int a = 0; a < 6; a++)
                for (int b2 = 0; b2 < 6; b2++) {
                    double sum = 0;
                    for (int s1 = 0; s1 < 3; s1++) for (int s2 = 0; s2 < 3; s2++) sum += J[s1][a] * Db[s1][s2] * J[s2][b2];
                    dI[li].m[a][b2] += h * sum;
                }
        }
    }
}

/* world pose and velocity of a point fixed in a link */
static void ta_point_state(const ta_kin* k, int link, const float* local, v3* p, v3* v) {
    v3 r = vf(local);
    *p = vadd(k->pw[link], mv(&k->Rw[link], r));
    *v = mv(&k->Rw[link], vadd(sv_lin(&k->v[link]), vcross(sv_ang(&k->v[link]), r)));
}
static void ta_geometry(const ppenv_config* c, const ta_kin* k, arm_geom* g) {
    int pl = c->paddle_link;
    ta_point_state(k, pl, c->paddle_center, &g->pc, &g->vpc);
    g->pn = mv(&k->Rw[pl], vf(c->paddle_normal));
    g->pnd = vcross(mv(&k->Rw[pl], sv_ang(&k->v[pl])), g->pn);
    for (int s = 0; s < c->num_shapes; s++) {
        ta_point_state(k, c->shape[s].link, c->shape[s].a, &g->sa[s], &g->va[s]);
        ta_point_state(k, c->shape[s].link, c->shape[s].b, &g->sb[s], &g->vb[s]);
    }
}

static void ta_write_row(float* row, v3 p, const m3* R, v3 lin, v3 ang) {
    double qt[4];
    rot_to_quat(R, qt);
    row[0] = (float)p.x; row[1] = (float)p.y; row[2] = (float)p.z;
    for (int t = 0; t < 4; t++) row[3 + t] = (float)qt[t];
    row[7] = (float)lin.x; row[8] = (float)lin.y; row[9] = (float)lin.z;
    row[10] = (float)ang.x; row[11] = (float)ang.y; row[12] = (float)ang.z;
}
/* rigid_body_states [42][13] of one env from its kinematics (gym.refresh_rigid_body_state_tensor) */
static void ta_body_states(const ppenv_ta_model* M, const ta_kin* k, const float* root /*[3][13]*/, float* rb) {
    for (int i = 0; i < TL; i++) {
        v3 lin = mv(&k->Rw[i], sv_lin(&k->v[i])), ang = mv(&k->Rw[i], sv_ang(&k->v[i]));
        ta_write_row(&rb[M->link[i].body * 13], k->pw[i], &k->Rw[i], lin, ang);
    }
    for (int f = 0; f < PPENV_TA_NUM_FIXED; f++) {
        const ppenv_ta_fixed* F = &M->fixed[f];
        v3 p, v;
        ta_point_state(k, F->link, F->xyz, &p, &v);
        m3 Rf = mf(F->rot), R = mm(&k->Rw[F->link], &Rf);
        ta_write_row(&rb[F->body * 13], p, &R, v, mv(&k->Rw[F->link], sv_ang(&k->v[F->link])));
    }
    memcpy(&rb[40 * 13], &root[13], 13 * sizeof(float));
    memcpy(&rb[41 * 13], &root[26], 13 * sizeof(float));
}

void ppo_ta_forward_kinematics(const ppenv_ta_model* M, int n, const float* root_states, const float* dof_states, float* rb_states) {
    for (int e = 0; e < n; e++) {
        double q[PPENV_TA_NUM_DOF], qd[PPENV_TA_NUM_DOF];
        for (int d = 0; d < PPENV_TA_NUM_DOF; d++) { q[d] = dof_states[((size_t)e * PPENV_TA_NUM_DOF + d) * 2]; qd[d] = dof_states[((size_t)e * PPENV_TA_NUM_DOF + d) * 2 + 1]; }
        ta_kin k;
        ta_kinematics(M, &root_states[(size_t)e * 39], q, qd, &k);
        ta_body_states(M, &k, &root_states[(size_t)e * 39], &rb_states[(size_t)e * 42 * 13]);
    }
}

static void ta_simulate_env(const ppenv_config* c, const ppenv_ta_model* M, const float* act, float* root /*[3][13]*/, float* dofs /*[27][2]*/,
                            float* rb, float* dof_force, float* pre_vx) {
    enum { NDF = PPENV_TA_NUM_DOF };
    double q[NDF], qd[NDF], target[NDF], tau_drive[NDF] = {0};
    for (int d = 0; d < NDF; d++) {
        const ppenv_ta_link* L = &M->link[d + 1];
        target[d] = pd_target(act[d], L->lower, L->upper, c->clip_actions);               /* TA:1131, 729-733 */
        q[d] = dofs[2 * d]; qd[d] = dofs[2 * d + 1];
    }
    float* ballf = &root[26];
    *pre_vx = ballf[7];                                                                    /* TA:1143 */
    ball_t b = {vf(&ballf[0]), vf(&ballf[7]), vf(&ballf[10])};
    double bq[4] = {ballf[3], ballf[4], ballf[5], ballf[6]};
    double pos[3] = {root[0], root[1], root[2]}, quat[4] = {root[3], root[4], root[5], root[6]};
    double vw[3] = {root[7], root[8], root[9]}, ww[3] = {root[10], root[11], root[12]};
    double h = (double)c->dt / c->substeps;
    sm6 I[TL];
    for (int i = 0; i < TL; i++) I[i] = spatial_inertia(M->link[i].mass, M->link[i].com, M->link[i].inertia);

    for (int s = 0; s < c->substeps; s++) {
        ta_kin k;
        ta_kinematics_d(M, pos, quat, vw, ww, q, qd, &k);
        sv6 fext[TL];
        sm6 dI[TL];
        ta_external(c, M, &k, h, fext, dI);

        /* drives */
        double tau[NDF], tau_lim[NDF], arm_eff[NDF];
        for (int d = 0; d < NDF; d++) {
            const ppenv_ta_link* L = &M->link[d + 1];
            double err = target[d] - q[d];
            /* implicit PD whose explicit part is clamped to the effort limit: continuous at saturation (the 7-dof arm's
             * spec switches branch there; on a floating base that switch would also be a momentum glitch) */
            tau[d] = clampd(L->kp * (err - h * qd[d]) - L->kd * qd[d], -L->effort, L->effort);
            arm_eff[d] = L->armature + h * L->kd + h * h * L->kp;
            tau_lim[d] = 0.0;
            double over = q[d] > L->upper ? q[d] - L->upper : (q[d] < L->lower ? q[d] - L->lower : 0.0);
            if (over != 0.0) {                       /* position limit: implicit spring-damper */
                /* limit spring with a quadratic toe over the first 0.01 rad (torque and stiffness start from zero: no jump at
                 * the limit); the implicit term uses the tangent stiffness, the damper fades in on the same ramp */
                double x = fabs(over), ramp = x < 0.01 ? x / 0.01 : 1.0;
                double phi = x < 0.01 ? x * x / 0.02 : x - 0.005;
                double kt = (double)M->limit_stiffness * ramp;
                tau_lim[d] += -(over > 0 ? 1.0 : -1.0) * (double)M->limit_stiffness * phi - kt * h * qd[d] - ramp * (double)M->limit_damping * qd[d];
                arm_eff[d] += h * (ramp * (double)M->limit_damping + h * kt);
            }
            if (fabs(qd[d]) > L->vel_limit) {        /* velocity limit: implicit damper on the excess, fading in over 1 rad/s */
                double ex = fabs(qd[d]) - L->vel_limit;
                tau_lim[d] += -(double)M->vel_limit_damping * (qd[d] > 0 ? ex : -ex);
                arm_eff[d] += h * (double)M->vel_limit_damping * (ex < 1.0 ? ex : 1.0);
            }
        }
        /* (M + diag) nu_dot = [0; tau] - C */
        static const double zero27[NDF] = {0};
        double A[TNV * TNV], rhs[TNV];
        sv6 f0, z6 = sv_zero();
        double tq[NDF];
        ta_rnea(M, &k, I, dI, fext, &z6, zero27, 1, &f0, tq);
        for (int t = 0; t < 6; t++) rhs[t] = -f0.a[t];
        for (int d = 0; d < NDF; d++) rhs[6 + d] = tau[d] + tau_lim[d] - tq[d];
        for (int col = 0; col < TNV; col++) {
            sv6 a0 = sv_zero();
            double qdd[NDF] = {0};
            if (col < 6) a0.a[col] = 1.0; else qdd[col - 6] = 1.0;
            ta_rnea(M, &k, I, dI, fext, &a0, qdd, 0, &f0, tq);
            for (int t = 0; t < 6; t++) A[t * TNV + col] = f0.a[t];
            for (int d = 0; d < NDF; d++) A[(6 + d) * TNV + col] = tq[d];
        }
        for (int d = 0; d < NDF; d++) A[(6 + d) * TNV + 6 + d] += arm_eff[d];
        solve_dense(TNV, A, rhs);

        /* ball against the start-of-substep geometry */
        arm_geom g;
        ta_geometry(c, &k, &g);
        const arm_geom* garr[1] = {&g};
        v3 bound = vadd(k.pw[M->bound_link], mv(&k.Rw[M->bound_link], vf(M->bound_center)));
        ball_substep_nb(c, &b, bq, 1, garr, &bound, h);

        /* integrate: base in world coordinates */
        v3 alpha = V(rhs[0], rhs[1], rhs[2]), ab = V(rhs[3], rhs[4], rhs[5]);
        v3 wb = sv_ang(&k.v[0]), vb = sv_lin(&k.v[0]);
        v3 aw = mv(&k.Rw[0], vadd(ab, vcross(wb, vb))), alw = mv(&k.Rw[0], alpha);
        vw[0] += h * aw.x; vw[1] += h * aw.y; vw[2] += h * aw.z;
        ww[0] += h * alw.x; ww[1] += h * alw.y; ww[2] += h * alw.z;
        for (int t = 0; t < 3; t++) pos[t] += h * vw[t];
        {
            double x = quat[0], y = quat[1], z = quat[2], w = quat[3], kq = 0.5 * h;
            double nx = x + kq * (ww[0] * w + ww[1] * z - ww[2] * y);
            double ny = y + kq * (ww[1] * w + ww[2] * x - ww[0] * z);
            double nz = z + kq * (ww[2] * w + ww[0] * y - ww[1] * x);
            double nw = w + kq * (-ww[0] * x - ww[1] * y - ww[2] * z);
            double nrm = sqrt(nx * nx + ny * ny + nz * nz + nw * nw);
            quat[0] = nx / nrm; quat[1] = ny / nrm; quat[2] = nz / nrm; quat[3] = nw / nrm;
        }
        for (int d = 0; d < NDF; d++) {
            const ppenv_ta_link* L = &M->link[d + 1];
            double err = target[d] - q[d];
            double v_new = qd[d] + h * rhs[6 + d];
            tau_drive[d] = clampd(L->kp * (err - h * v_new) - L->kd * v_new, -L->effort, L->effort);
            q[d] += h * v_new; qd[d] = v_new;   /* limits act through tau_lim: no clamp */
        }
    }
    /* refresh: round to the fp32 tensors */
    for (int t = 0; t < 3; t++) { root[t] = (float)pos[t]; root[7 + t] = (float)vw[t]; root[10 + t] = (float)ww[t]; }
    for (int t = 0; t < 4; t++) root[3 + t] = (float)quat[t];
    for (int d = 0; d < NDF; d++) { dofs[2 * d] = (float)q[d]; dofs[2 * d + 1] = (float)qd[d]; dof_force[d] = (float)tau_drive[d]; }
    ballf[0] = (float)b.p.x; ballf[1] = (float)b.p.y; ballf[2] = (float)b.p.z;
    for (int t = 0; t < 4; t++) ballf[3 + t] = (float)bq[t];
    ballf[7] = (float)b.v.x; ballf[8] = (float)b.v.y; ballf[9] = (float)b.v.z;
    ballf[10] = (float)b.w.x; ballf[11] = (float)b.w.y; ballf[12] = (float)b.w.z;
    double qf[NDF], qdf[NDF];
    for (int d = 0; d < NDF; d++) { qf[d] = dofs[2 * d]; qdf[d] = dofs[2 * d + 1]; }
    ta_kin kf;
    ta_kinematics(M, root, qf, qdf, &kf);
    ta_body_states(M, &kf, root, rb);
}

/* Domain randomisation of the 27-DoF step (include/ppenv.h ppenv_ta_randomization; the yaml's randomization_params block, identical in every task
 * yaml): as for the 3-actor step every env gets its OWN copy of the model and of the scene with its table entries applied — drive gains, link masses
 * (inertia with them), restitution / friction of the humanoid's shapes and the paddle — and the action noise is added to the raw actions before the
 * clamp.  The noise index space of this task is 512 wide (27 action draws, then 32 + k for observation value k < 313): folded into dr_gauss's
 * 256-per-step keys as (2 progress + index / 256, index % 256); the kernel (ppenv_ta_chain.hip ta_dr_gauss) does the same. */
static float ta_dr_gauss(uint64_t seed, uint32_t gid, uint32_t episode, uint32_t progress, uint32_t index) {
    return dr_gauss(seed, gid, episode, 2u * progress + (index >> 8), index & 255u);
}
void ppo_ta_simulate_dr(const ppenv_config* c, const ppenv_ta_model* M, int n, int threads, const float* actions, float* root_states,
                        float* dof_states, float* rb_states, float* dof_force, float* pre_ball_vx, const float* kp_scale /*[27][n]*/,
                        const float* kd_scale /*[27][n]*/, const float* mass_scale /*[28][n]*/, const float* e_scale /*[n]*/, const float* mu_scale /*[n]*/,
                        float action_sigma, uint64_t seed, int env_id_offset, const uint32_t* episode, const int64_t* progress) {
#ifdef _OPENMP
#pragma omp parallel for num_threads(threads > 0 ? threads : 1) schedule(static)
#endif
    for (int e = 0; e < n; e++) {
        ppenv_ta_model Me = *M;
        ppenv_config ce = *c;
        for (int i = 0; i < PPENV_TA_NUM_LINKS; i++) {
            ppenv_ta_link* L = &Me.link[i];
            if (i > 0 && kp_scale) L->kp *= kp_scale[(size_t)(i - 1) * n + e];
            if (i > 0 && kd_scale) L->kd *= kd_scale[(size_t)(i - 1) * n + e];
            if (mass_scale) {
                float sc = mass_scale[(size_t)i * n + e];
                L->mass *= sc;
                for (int k = 0; k < 6; k++) L->inertia[k] *= sc;
            }
        }
        float es = e_scale ? e_scale[e] : 1.f, fs = mu_scale ? mu_scale[e] : 1.f;
        ce.paddle_restitution = fminf(ce.paddle_restitution * es, ce.restitution_max); ce.paddle_friction *= fs;
        for (int sh = 0; sh < ce.num_shapes; sh++) { ce.shape[sh].restitution = fminf(ce.shape[sh].restitution * es, ce.restitution_max); ce.shape[sh].friction *= fs; }
        float act[PPENV_TA_NUM_DOF];
        for (int d = 0; d < PPENV_TA_NUM_DOF; d++) {
            act[d] = actions[(size_t)e * PPENV_TA_NUM_DOF + d];
            if (action_sigma > 0.f) act[d] += action_sigma * ta_dr_gauss(seed, (uint32_t)(env_id_offset + e), episode[e], (uint32_t)progress[e], (uint32_t)d);
        }
        ta_simulate_env(&ce, &Me, act, &root_states[(size_t)e * 39], &dof_states[(size_t)e * 54],
                        &rb_states[(size_t)e * 42 * 13], &dof_force[(size_t)e * PPENV_TA_NUM_DOF], &pre_ball_vx[e]);
    }
}
/* observation noise: added to the finished rows, keyed by the episode / progress the step STARTED with */
void ppo_ta_add_obs_noise(float* obs /*[n,313]*/, int n, float sigma, uint64_t seed, int env_id_offset, const uint32_t* episode0, const int64_t* progress0) {
    if (!(sigma > 0.f)) return;
    for (int e = 0; e < n; e++)
        for (int k = 0; k < PPENV_TA_NUM_OBS; k++)
            obs[(size_t)e * PPENV_TA_NUM_OBS + k] += sigma * ta_dr_gauss(seed, (uint32_t)(env_id_offset + e), episode0[e], (uint32_t)progress0[e], 32u + (uint32_t)k);
}

void ppo_ta_simulate(const ppenv_config* c, const ppenv_ta_model* M, int n, int threads, const float* actions, float* root_states,
                     float* dof_states, float* rb_states, float* dof_force, float* pre_ball_vx) {
#ifdef _OPENMP
#pragma omp parallel for num_threads(threads > 0 ? threads : 1) schedule(static)
#endif
    for (int e = 0; e < n; e++)
        ta_simulate_env(c, M, &actions[(size_t)e * PPENV_TA_NUM_DOF], &root_states[(size_t)e * 39], &dof_states[(size_t)e * 54],
                        &rb_states[(size_t)e * 42 * 13], &dof_force[(size_t)e * PPENV_TA_NUM_DOF], &pre_ball_vx[e]);
}
