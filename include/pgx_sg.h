/*
 * pgx_sg.h - C ABI of libpgx.so for the LVPP Newton inner loop of example 02 (Signorini contact of a 3-D - or, through
 * pgx_sg_create_2d below, plane - linear-elastic body with a rigid plane; latent variable on the contact surface): everything below `solver.solve()` in
 * examples/02_signorini/signorini_dolfinx.py:333, i.e. what the reference delegates to DOLFINx assembly (cell + exterior
 * facet integrals on a submesh, :199-249) + PETSc SNES (newtonls, linesearch none) + MUMPS LU (:271-291).
 *
 * Spaces at degree 1 (BASELINE.json config 5): u in (P1)^3 on a tetrahedral mesh, psi in P1 on the contact facets; degree 2 (the
 * reference's default, :68-73; pgx_sg_mesh.degree = 2): u in (P2)^3, psi in P2 on the contact facets, affine cells; hexahedra
 * (the reference's native mesh, :376-383; pgx_sg_mesh.cell_type = 1) with Q1 / Q2 elements on parallelepipeds.
 *        x = [u_x (nv) | u_y (nv) | u_z (nv) | psi (one per contact node, ordered by node id)],  nv = vertices (degree 1) / P2 nodes
 * Residual (:236-249), n_g = -e_z, g = x_z - gap, f = 0:
 *        R_u   = alpha (sigma(u), eps(v)) - <psi - psi_k, v.n_g>_Gamma
 *        R_psi = <u.n_g, w>_Gamma + <exp(psi), w>_Gamma - <g, w>_Gamma
 * Jacobian [[alpha A, +M_G],[-M_G, D(psi)]] (nonsymmetric sign pattern, as UFL's derivative gives it).
 *
 *   pgx_sg_create         NonlinearProblem(F, [u, psi], bcs, entity_maps, petsc_options) construction (:281-291)
 *   pgx_sg_set/get_state, pgx_sg_set/get_prev, pgx_sg_advance_prev   u.x.array / psi.x.array / psi_k, u_prev (:336-343)
 *   pgx_sg_set_alpha      alpha.value = ... (:323-328)
 *   pgx_sg_residual / pgx_sg_jacobian_fill / pgx_sg_csr_export / pgx_sg_spmv   SNES callbacks and the PETSc Mat
 *   pgx_sg_newton_solve   solver.solve() (:333) with reason / iteration count (:334-335); tolerances as set by
 *                         solver.solver.setTolerances(atol=, rtol=) (:331-332)
 *   pgx_sg_u_increment    ||u - u_prev||_2 (vector 2-norm, :337-339)
 *   pgx_sg_penetration / pgx_sg_violation / pgx_sg_von_mises   what the script reports about an iterate (:293-321, 346-350)
 * Conventions as in pgx.h.  Linear solves: sparse LU of pgx_nd.h + iterative refinement.  No CPU fallback.
 */
#ifndef PGX_SG_H
#define PGX_SG_H
#include <stdint.h>

#include "pgx.h"
#include "pgx_nd.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct pgx_sg_handle pgx_sg_handle;

typedef struct {
  int32_t n_vertices, n_cells;
  const double* coords;    /* [n_vertices][3] */
  const int32_t* cells;    /* [n_cells][4] */
  int32_t n_facets;        /* potential-contact facets (facet_tag.find(contact), :186-189) */
  const int32_t* facets;   /* [n_facets][3] vertex ids */
  int32_t degree;          /* 0 or 1: degree 1 as described above.  2 (the reference's default, :68-73): u in (P2)^3, psi in P2 on the
                            * contact facets.  Then n_vertices counts the P2 NODES (mesh vertices, then one node per edge; `coords`
                            * holds the edge midpoints for them), cells is [n_cells][10]: 4 vertices, then the edge nodes of
                            * (0,1) (0,2) (0,3) (1,2) (1,3) (2,3); facets is [n_facets][6]: 3 vertices, then the edge nodes of
                            * (0,1) (0,2) (1,2).  Cells are affine (geometry from the vertices) unless created by pgx_sg_create_curved.  bc_dofs: component * n_nodes +
                            * node; pgx_sg_contact_vertices returns the node of every psi dof. */
  int32_t cell_type;       /* 0: tetrahedra (above).  1: hexahedra - the reference's native mesh (:376-383) - with Q_d elements, d = degree
                            * (0 / 1 -> Q1, 2 -> Q2): cells is [n_cells][(d+1)^3], facets [n_facets][(d+1)^2] (quadrilaterals), local nodes
                            * numbered lexicographically (xi fastest), basis = tensor Lagrange on the equispaced nodes k/d; cells and facets
                            * must be affine images of the cube / square (parallelepipeds: true for box grids).  The facet quadrature of
                            * pgx_sg_problem is then a rule on the unit SQUARE (weights sum to 1). */
} pgx_sg_mesh;

typedef struct {
  double E, nu, gap;       /* :58-66 */
  int32_t nq;              /* facet quadrature (degree 4 in the reference, :67-69), <= 16 points */
  const double* qpts;      /* [nq][2] reference triangle */
  const double* qwts;      /* [nq], sum 1/2 */
  int32_t n_bc;            /* Dirichlet dofs of u: component * n_vertices + vertex (:255-268) */
  const int32_t* bc_dofs;
  const double* bc_vals;   /* NULL = homogeneous */
} pgx_sg_problem;

int pgx_sg_create(const pgx_sg_mesh* mesh, const pgx_sg_problem* prob, int device, pgx_sg_handle** out);
/* PLANE PROBLEMS: the script with gdim = 2 (`native --dim 2`: create_unit_square(nx, ny, quadrilateral), :376-380; `file`: the half disk
 * of lvpp.mesh_generation.create_half_disk).  Every expression of the script is written against gdim, so
 *        x = [u_x (nv) | u_y (nv) | psi (one per contact node, ordered by node id)],   n_g = -e_y,  g = x_y - gap,  f = 0,
 * Jacobian [[alpha A, +M_G],[-M_G, D(psi)]], BC dofs component * n_nodes + node, and mu, lambda EXACTLY the script's (:234-235) - the
 * plane-strain operator; plane-stress constants are NOT substituted.  pgx_sg_create_2d returns the same pgx_sg_handle: every call
 * below works on it with gdim = 2 (pgx_sg_violation: -u_y - (y - gap); pgx_sg_u_increment: over the 2 nv displacement dofs).
 * pgx_sg_create_dist and pgx_sg_create_curved stay 3-D ONLY: there is no distributed and no curved plane handle.
 *
 * Elements, all on AFFINE cells (PGX_EINVAL otherwise: straight-sided triangles with their edge nodes at the midpoints;
 * quadrilaterals must be parallelograms with their nodes on the lattice, as the hexahedral path requires parallelepipeds):
 *   cell_type 0, degree 1:  cells [n_cells][3];  contact edges [n_facets][2]
 *   cell_type 0, degree 2:  cells [n_cells][6]: 3 vertices, then the edge nodes of (0,1) (0,2) (1,2) - the 3-D facet convention; basis
 *                           L_a (2 L_a - 1), 4 L_a L_b;  contact edges [n_facets][3]: the two vertices, then the midpoint node; basis on
 *                           t in [0,1]: (1 - t)(1 - 2t), t (2t - 1), 4 t (1 - t)
 *   cell_type 1, degree 1:  cells [n_cells][4], local nodes lexicographic (xi fastest);  contact edges [n_facets][2]
 *   cell_type 1, degree 2:  cells [n_cells][9], lexicographic, tensor Lagrange on the nodes k/2 as the hexahedral path;  contact edges
 *                           [n_facets][3], lexicographic (end, midpoint, end)
 * n_vertices counts the NODES of the discretisation, coords holds all of them.  Quadrature: contact edges - the caller's rule on
 * [0,1] (weights sum to 1; the binding passes basix's default for the script's quadrature_degree: Gauss-Legendre with
 * (degree + 2) / 2 points, 3 at the default 4); the edge length is the surface element.  Cells - triangles: the centroid (degree 1,
 * constant integrand) / the 3-point degree-2 rule (1/6,1/6) (2/3,1/6) (1/6,2/3), weights 1/6 (degree 2: exact, gradients are affine);
 * quadrilaterals: Gauss-Legendre (d + 1)^2 on the unit square.  (UFL's own estimate of the cell degree on quadrilaterals is not
 * reproduced: the rule here is exact for Q1 and Q2 on parallelograms.) */
typedef struct {
  int32_t n_vertices, n_cells;
  const double* coords;    /* [n_vertices][2] */
  const int32_t* cells;    /* [n_cells][3 | 6 | 4 | 9] */
  int32_t n_facets;        /* potential-contact edges */
  const int32_t* facets;   /* [n_facets][2 | 3] node ids */
  int32_t degree;          /* 0 or 1: degree 1; 2: degree 2 */
  int32_t cell_type;       /* 0: triangles, 1: quadrilaterals */
} pgx_sg_mesh2d;
typedef struct {
  double E, nu, gap;
  int32_t nq;              /* edge quadrature, <= 16 points */
  const double* qpts;      /* [nq] on [0,1] */
  const double* qwts;      /* [nq], sum 1 */
  int32_t n_bc;            /* Dirichlet dofs of u: component * n_vertices + node, component 0 or 1 */
  const int32_t* bc_dofs;
  const double* bc_vals;   /* NULL = homogeneous */
} pgx_sg_problem2d;
int pgx_sg_create_2d(const pgx_sg_mesh2d* mesh, const pgx_sg_problem2d* prob, int device, pgx_sg_handle** out);
/* ORDER-2 GEOMETRY (round 5): the reference's half sphere is a mesh of 10-node tetrahedra (src/lvpp/mesh_generation.py:88,158
 * `order=2`) and DOLFINx integrates on the curved cells.  With pgx_sg_mesh.degree = 2 the ten nodes of a cell ARE its geometry nodes
 * (`coords` of an edge node = the mesh's mid-edge node instead of the midpoint): the discretisation is isoparametric P2; with degree 1
 * the mesh arrays hold the vertices only (P1 fields on the quadratic cells).  In both cases the geometry itself enters through two
 * tables a binding reads off the coordinate element: */
typedef struct {
  int32_t nq;              /* cell quadrature on the reference tetrahedron (weights sum 1/6).  The reference leaves this integral's
                            * degree to UFL's estimator (signorini_dolfinx.py:237-239 has no metadata on dx); <= 512 points */
  const double* qpts;      /* [nq][3] */
  const double* qwts;      /* [nq] */
  const double* cell_geo;  /* [n_cells][nq][10]: |det J|, then J^-1 row-major (d xi_k / d x_d) of x(xi) = sum_a X_a N2_a(xi) */
  const double* facet_geo; /* [n_facets][prob->nq][2]: surface element |x_xi x x_eta| of the 6-node contact facet and its z
                            * coordinate at the facet quadrature points of pgx_sg_problem */
} pgx_sg_curved;
/* Single handle, tetrahedra, degree 1 or 2 (PGX_EINVAL otherwise).  Everything else as pgx_sg_create. */
int pgx_sg_create_curved(const pgx_sg_mesh* mesh, const pgx_sg_problem* prob, const pgx_sg_curved* curved, int device,
                         pgx_sg_handle** out);
/* One handle per GPU over a pgx_comm (BASELINE.json config 5: 4 GPUs).  The ELEMENTS are partitioned (round 4): the cells are cut
 * into comm->size slabs of equal count along the longest axis of the mesh, every rank assembles the elasticity blocks of its own
 * slab only and one all-reduce sums the constant matrix - the owned-cell assembly of a distributed DOLFINx mesh
 * (signorini_dolfinx.py:283-291, `kind="mpi"`); the sparse LU, 94 % of a Newton step, is distributed (pgx_nd_create_dist).  Still
 * replicated: the mesh arrays handed in, the iterate, and what a Newton step assembles on top of the constant matrix (a product
 * with it and the contact facets: < 1 % of a step).  Replaces `mpirun -n N python signorini_dolfinx.py`; all calls are collective
 * and return identical results on every rank.  Tuning key PGX_SG_PARTITION=0: every rank assembles every cell (rounds 2-3). */
int pgx_sg_create_dist(const pgx_sg_mesh* mesh, const pgx_sg_problem* prob, pgx_comm* comm, int device, pgx_sg_handle** out);
/* cells whose element matrices THIS rank assembled / cells of the mesh (equal on a single handle) */
int pgx_sg_partition_info(const pgx_sg_handle* h, int64_t* owned_cells, int64_t* total_cells);
/* symbolic statistics of the handle's sparse LU (flop counts, arena size: include/pgx_nd.h) */
int pgx_sg_lu_stats(const pgx_sg_handle* h, pgx_nd_stats* st);
/* 1: the handle's sparse LU runs in symmetric mode (the latent rows are negated on the way into it: csrc/pgx_mixed.hip mx_lu_factor) */
int pgx_sg_lu_is_symmetric(const pgx_sg_handle* h);
void pgx_sg_destroy(pgx_sg_handle* h);
const char* pgx_sg_last_error(const pgx_sg_handle* h);
int pgx_sg_num_dofs(const pgx_sg_handle* h, int64_t* ntot, int64_t* npsi);
int pgx_sg_contact_vertices(const pgx_sg_handle* h, int32_t* verts /* [npsi]: vertex of each psi dof */);
int pgx_sg_set_state(pgx_sg_handle* h, const double* x);
int pgx_sg_get_state(pgx_sg_handle* h, double* x);
int pgx_sg_set_prev(pgx_sg_handle* h, const double* x);
int pgx_sg_get_prev(pgx_sg_handle* h, double* x);
int pgx_sg_advance_prev(pgx_sg_handle* h);
int pgx_sg_set_alpha(pgx_sg_handle* h, double alpha);
int pgx_sg_residual(pgx_sg_handle* h, const double* x, double* F, double* fnorm);
int pgx_sg_jacobian_fill(pgx_sg_handle* h, const double* x);
int pgx_sg_csr_export(pgx_sg_handle* h, int64_t* nrows, int64_t* nnz, int32_t* rowptr, int32_t* col, double* vals);
int pgx_sg_spmv(pgx_sg_handle* h, const double* x, double* y);
int pgx_sg_newton_solve(pgx_sg_handle* h, const pgx_snes_opts* opts, int* reason, int* its, int* lin_its);
int pgx_sg_u_increment(pgx_sg_handle* h, double* out);
/* Diagnostics of the device state h->x: one pass each, no handle state changes (a Jacobian filled before stays valid).  On a handle
 * of pgx_sg_create_dist they run on the rank's replica of the iterate WITHOUT communication and so need not be called collectively
 * (untested on more than one rank). */
/* sqrt( int_Gamma max(u.n_g - g, 0)^2 ds ), n_g = -e_z, g = x_z - gap, with the facet rule of pgx_sg_problem (:307-314); curved handles:
 * surface element and z from pgx_sg_curved.facet_geo.  Fixed-shape reduction: bitwise reproducible. */
int pgx_sg_penetration(pgx_sg_handle* h, double* l2);
/* u.n_g - g = -u_z - (z - gap) (plane handles: -u_y - (y - gap)) at every node (Expression at V's interpolation points, :307-308, 349) */
int pgx_sg_violation(pgx_sg_handle* h, double* out /* [n_nodes] */);
/* sqrt(3/2 s:s), s = sigma(u) - tr(sigma(u))/3 I, at the cell's own nodes = DG_degree interpolation (:296-302, 346).  Affine cells of all
 * four element flavours.  Plane handles: the SCRIPT'S expression with len(u) = 2, i.e. the 2 x 2 sigma and
 * s = sigma - tr(sigma)/3 I_2 (:300-301) - this is NOT the plane-strain von Mises stress (no sigma_zz, and the 1/3 stays).  LIMITATION: PGX_EINVAL on a handle of pgx_sg_create_curved - it holds the cell geometry at the quadrature
 * points only, not at the nodes. */
int pgx_sg_von_mises(pgx_sg_handle* h, double* out /* [n_cells][nodes per cell], the node order of pgx_sg_mesh.cells */);
int pgx_sg_profile(pgx_sg_handle* h, int enable, double ms[6]);

#ifdef __cplusplus
}
#endif
#endif
