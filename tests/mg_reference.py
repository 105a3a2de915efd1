"""fp64 restatement of the multigrid level operators, with a magnitude pass for componentwise error bounds.

Inputs are only what the C ABI exports: a level's padded ELL matrix (`ctx.matrix(l)`), its node coordinates
(`ctx.level(l)["id2coord"]`) and the prolongation (`ctx.prolongation(l)`).  Every operator returns its fp64 value and a
per-component magnitude `m`, and a correct implementation in unit round-off u satisfies

    |got - ref| <= K u m        componentwise,

with K a count of the rounded operations a component depends on (the K_* constants and k_* functions below).  Rows of low-mass
boundary nodes, whose entries are 1e-8 of the largest, are held to their own scale, not to the largest entry's.

Single operations (SpMV, P x, P^T x, P^T A P): m is the same computation on absolute values (|A| |x|, |P| |x|, |P|^T |A| |P|), and
the bound is the standard first-order one (Higham, "Accuracy and Stability of Numerical Algorithms", 2nd ed., section 3.1): a sum of
s products carries at most s u of the sum of the products' absolute values, in any order, plus u for the products.

Iterations (the smoothers, the V-cycle): m is the sum of the LOCAL magnitudes of the steps that produced a component — each step's
absolute-value computation on the actual values of its operands (a substitution step D^-1 (r - sum A x): |D^-1| |D| |D^-1| (|r| +
sum |A| |x|), because an implementation forms D^-1 in its working precision).  Carrying absolute values through a whole substitution
chain instead (|D^-1| |A| applied 512 times) grows geometrically on these matrices, which are not diagonally dominant, and bounds
nothing; with local magnitudes an error made upstream reaches a row through the signed operator, and K counts the dependent steps
of the chain (GS_GROUPS per half sweep).  tests/test_oracle_mg_reference.py shows that the oracle's own float arithmetic meets
these bounds: K is derived, not fitted to the device.

The smoother order is the reference's (oracle/sim_matrix.hpp mark_colors; tests/golden/np_step.py gs_order): 4^3 blocks,
colour = parity bits of the block coordinates, blocks numbered per colour in first-touch order, rows in id order inside a block.
Blocks of one colour are at least five nodes apart and a row couples to nodes at most two away, so the rows of one colour that
share their position inside their blocks are independent: the sweeps below update them together, (colour, position) group by
group, which is the sequential sweep exactly."""
import numpy as np

U64, U32 = 2.0 ** -53, 2.0 ** -24

# ---- constants K (first-order error counts) and their derivations
K_SPMV = 3 * 126 + 1  # a row of A x: at most 126 slots x 3 components summed, plus the products' own rounding
K_PROLONG = 8 + 1  # a row of P x: 8 weights
K_RESTRICT = 27 + 1  # a row of P^T x: a coarse node collects at most 3^3 fine nodes
K_GALERKIN = 27 * 27 * 3 + 2  # (P^T A P)_ab: at most 27 x 27 fine pairs x 3 components, each a product of three
K_INV3 = 16  # a 3x3 inverse from cofactors and the determinant, relative to |D^-1| |D| |D^-1|
K_ROW = K_SPMV + 1 + 3 + K_INV3  # one substitution step D^-1 (r - sum A x): the row sum, the difference, the 3x3 product, the inverse
GS_GROUPS = 8 * 64  # dependent steps of a half sweep: (colour, position in a 4^3 block) groups; the rows of a group are independent


def k_gs(iterations):
    """kind 5 after `iterations` (rounded up to symmetric sweeps): two half sweeps of GS_GROUPS dependent substitution steps, the
    diagonal scaling between them, u += du and r -= A du — per sweep, the sweeps' errors enter the next one through r"""
    return ((iterations + 1) >> 1) * (2 * GS_GROUPS * K_ROW + 3 + K_SPMV + 1)


def k_jacobi(iterations):
    """kinds 0 / 1: du = D^-1 r (3 terms and the inverse), dA u (K_SPMV), two dot products (their relative error is carried by the
    magnitude pass's condition factors), the updates"""
    return iterations * (3 + K_INV3 + K_SPMV + 4)


def k_pcg(iterations):
    """kind 2: per iteration a product (K_SPMV), the preconditioner (3 + K_INV3), three updates; the dot products as for k_jacobi"""
    return (iterations + 1) * (K_SPMV + 3 + K_INV3 + 6)


def ratio(got, ref, m, u):
    """largest |got - ref| / (u m) (components with m = 0 must match exactly: reported as inf otherwise)"""
    got, ref, m = (np.asarray(a, np.float64) for a in (got, ref, m))
    d = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(m > 0, d / (u * m), np.where(d > 0, np.inf, 0.0))
    return float(q.max()) if q.size else 0.0


def normwise(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300))


def gs_keys(coord):
    """(colour, block id in first-touch order within the colour, 0-based position in the block) of every node"""
    coord = np.asarray(coord, np.int64)
    b = coord >> 2
    colour = ((b[:, 0] & 1) << 2) | ((b[:, 1] & 1) << 1) | (b[:, 2] & 1)
    bmin = b.min(0)
    bkey = ((b[:, 0] - bmin[0]) * (1 << 21) + (b[:, 1] - bmin[1])) * (1 << 21) + (b[:, 2] - bmin[2])
    uk, first, inv = np.unique(bkey, return_index=True, return_inverse=True)
    inv = inv.ravel()
    ucol = colour[first]
    # block id per colour: rank of the block's first row among the colour's blocks
    bid_of_block = np.empty(len(uk), np.int64)
    for c in range(8):
        sel = np.nonzero(ucol == c)[0]
        bid_of_block[sel[np.argsort(first[sel], kind="stable")]] = np.arange(len(sel))
    blk = inv
    order = np.lexsort((np.arange(len(coord)), blk))  # rows grouped by block, id order inside
    start = np.zeros(len(uk) + 1, np.int64)
    np.add.at(start, blk + 1, 1)
    start = np.cumsum(start)
    pos = np.empty(len(coord), np.int64)
    pos[order] = np.arange(len(coord)) - start[blk[order]]
    return colour, bid_of_block[blk], pos


class Level:
    """One level: A as an (n, 3, 3 colsize) row-block array in the smoother's group order (fp64), its column indices, the 3x3
    diagonal blocks and their fp64 inverses."""

    def __init__(self, col, val, coord, chunk=16384):
        col = np.asarray(col)
        n, k = col.shape
        self.n = n
        colour, bid, pos = gs_keys(coord)
        self.colour_blocks = [int(bid[colour == c].max()) + 1 if (colour == c).any() else 0 for c in range(8)]
        self.perm = np.lexsort((bid, pos, colour))  # groups (colour, position) contiguous
        g = colour[self.perm] * 64 + pos[self.perm]
        cut = np.nonzero(np.diff(g))[0] + 1
        self.groups = list(zip(np.r_[0, cut], np.r_[cut, n]))
        self.col = np.ascontiguousarray(col[self.perm])
        self.W = np.empty((n, 3, 3 * k))
        D = np.zeros((n, 3, 3))
        for a in range(0, n, chunk):
            rows = self.perm[a:a + chunk]
            V = np.asarray(val[rows], np.float64).reshape(len(rows), k, 3, 3)  # column-major 3x3: V[i, s, c, r] = A_s[r][c]
            self.W[a:a + chunk] = V.transpose(0, 3, 1, 2).reshape(len(rows), 3, 3 * k)
            self_ = (col[rows] == rows[:, None])
            D[rows] = np.einsum("is,iscr->irc", self_.astype(np.float64), V)
        self.aW = np.abs(self.W)
        self.D = D
        self.aD = np.abs(D)
        self.Dinv = np.linalg.inv(D)
        self.aDinv = np.abs(self.Dinv)
        self.G = np.einsum("iab,ibc,icd->iad", self.aDinv, self.aD, self.aDinv)  # |D^-1| |D| |D^-1|

    # products of the rows perm[a:b] (results in that order)
    def _rows(self, W, a, b, x):
        xg = x[self.col[a:b]].reshape(b - a, -1, 1)
        return np.matmul(W[a:b], xg)[:, :, 0]

    def mul(self, x, W=None, chunk=16384):
        W = self.W if W is None else W
        x = np.asarray(x, np.float64)
        y = np.empty((self.n, 3))
        for a in range(0, self.n, chunk):
            b = min(self.n, a + chunk)
            y[self.perm[a:b]] = self._rows(W, a, b, x)
        return y

    def spmv(self, x):
        """(A x, |A| |x|)"""
        return self.mul(x), self.mul(np.abs(x), self.aW)

    def dense(self, chunk=8192):
        """A as a scipy CSR matrix (the exported slots summed, zero slots dropped)"""
        import scipy.sparse as sp
        n, k3 = self.n, self.W.shape[2]
        parts = []
        for a in range(0, n, chunk):
            W = self.W[a:a + chunk]
            i, r, s = np.nonzero(W)
            c = 3 * self.col[a + i, s // 3] + s % 3
            parts.append(sp.csr_matrix((W[i, r, s], ((3 * i + r).astype(np.int64), c.astype(np.int64))), shape=(3 * len(W), 3 * n)))
        inv = np.empty(n, np.int64)
        inv[self.perm] = np.arange(n)
        rows = (3 * inv[:, None] + np.arange(3)[None, :]).ravel()
        return sp.vstack(parts).tocsr()[rows]

    # ---- smoothers (oracle/sim_matrix.hpp Sim::smooth)
    def scale(self, x, m, Ainv=1):
        """D^-1 x (Ainv 1: the 3x3 block inverse; 0: the inverse diagonal entries) and its magnitude"""
        if Ainv == 0:
            d = np.einsum("iaa->ia", self.D)
            return x / d, m / np.abs(d)
        return np.einsum("iab,ib->ia", self.Dinv, x), np.einsum("iab,ib->ia", self.G, m)

    def gs(self, u, r, iterations, mu=None, mr=None):
        """kind 5: symmetric coloured block GS, (iterations + 1) >> 1 sweeps; returns (u, r, m_u, m_r)"""
        u, r = np.array(u, np.float64), np.array(r, np.float64)
        mu = np.abs(u) if mu is None else np.array(mu, np.float64)
        mr = np.abs(r) if mr is None else np.array(mr, np.float64)
        n, P = self.n, self.perm
        for _ in range((iterations + 1) >> 1):
            h, mh = np.zeros((n, 3)), np.zeros((n, 3))
            ar = np.abs(r)
            for a, b in self.groups:
                rows = P[a:b]
                s = self._rows(self.W, a, b, h)
                h[rows] = np.einsum("iab,ib->ia", self.Dinv[rows], r[rows] - s)
                mh[rows] = np.einsum("iab,ib->ia", self.G[rows], ar[rows] + self._rows(self.aW, a, b, np.abs(h)))
            hd = np.einsum("iab,ib->ia", self.D, h)
            ahd = np.maximum(np.abs(hd), np.einsum("iab,ib->ia", self.aD, mh))
            du, mdu = np.zeros((n, 3)), np.zeros((n, 3))
            for a, b in reversed(self.groups):
                rows = P[a:b]
                s = self._rows(self.W, a, b, du)
                du[rows] = np.einsum("iab,ib->ia", self.Dinv[rows], hd[rows] - s)
                mdu[rows] = np.einsum("iab,ib->ia", self.G[rows], ahd[rows] + self._rows(self.aW, a, b, np.abs(du)))
            u, mu = u + du, mu + mdu
            r, mr = r - self.mul(du), mr + self.mul(mdu, self.aW)
        return u, r, mu, mr

    def jacobi(self, u, r, iterations, kind, topomega=0.1, tolerance=0.0, Ainv=1):
        """kind 0 (damped by topomega) and kind 1 (optimal step); returns (u, r, m_u, m_r)"""
        u, r = np.array(u, np.float64), np.array(r, np.float64)
        mu, mr = np.abs(u), np.abs(r)
        for _ in range(iterations):
            if kind == 1 and np.sqrt((r * r).sum()) < tolerance:
                break
            du, mdu = self.scale(r, np.abs(r), Ainv)
            if kind == 0:
                du, mdu = du * topomega, mdu * topomega
                u, mu, r, mr = u + du, mu + mdu, r - self.mul(du), mr + self.mul(mdu, self.aW)
                continue
            dAu, mdAu = self.mul(du), self.mul(mdu, self.aW)
            a, b = (du * r).sum(), (du * dAu).sum()
            om = a / b
            kap = _cond(du, r, a) + _cond(du, dAu, b)  # relative error of omega in units of u (the two dot products)
            u, mu = u + om * du, mu + abs(om) * (mdu + kap * np.abs(du))
            r, mr = r - om * dAu, mr + abs(om) * (mdAu + kap * np.abs(dAu))
        return u, r, mu, mr

    def pcg(self, u, r, iterations, r0=None, Ainv=1):
        """kind 2: PCG with the block-diagonal preconditioner, stopped once z.r < 0.25 z0.r0 of the initial residual r0;
        returns (u, r, m_u, m_r, iterations taken, the last z.r / tolerance)"""
        u, r = np.array(u, np.float64), np.array(r, np.float64)
        r0 = r.copy() if r0 is None else np.asarray(r0, np.float64)
        mu, mr = np.abs(u), np.abs(r)
        z, _ = self.scale(r0, np.abs(r0), Ainv)
        tol = (z * r0).sum() * 0.25
        z, mz = self.scale(r, np.abs(r), Ainv)
        du, mdu = z.copy(), mz.copy()
        ztr = (z * r).sum()
        kz = _cond(z, r, ztr)
        cnt = 0
        for _ in range(iterations):
            if ztr < tol:
                break
            dAu, mdAu = self.mul(du), self.mul(mdu, self.aW)
            den = (dAu * du).sum()
            om = ztr / den
            kap = kz + _cond(dAu, du, den)
            u, mu = u + om * du, mu + abs(om) * (mdu + kap * np.abs(du))
            r, mr = r - om * dAu, mr + abs(om) * (mdAu + kap * np.abs(dAu))
            z, mz = self.scale(r, np.abs(r), Ainv)
            pre, ztr = ztr, (z * r).sum()
            kz_pre, kz = kz, _cond(z, r, ztr)
            beta = ztr / pre
            du, mdu = z + beta * du, mz + abs(beta) * (mdu + (kz + kz_pre) * np.abs(du))
            cnt += 1
        return u, r, mu, mr, cnt, ztr / tol if tol != 0 else np.inf


def _cond(a, b, ab):
    """relative condition of the dot product a.b (sum |a||b| / |a.b|)"""
    return float((np.abs(a) * np.abs(b)).sum() / max(abs(ab), 1e-300))


class Transfer:
    """The trilinear prolongation P between level l (fine, rows) and level l + 1 (coarse, columns), from ctx.prolongation(l)"""

    def __init__(self, pcol, pw, ncoarse):
        import scipy.sparse as sp
        pcol = np.asarray(pcol)
        nf = pcol.shape[0]
        w = np.asarray(pw, np.float64).ravel()
        self.P = sp.coo_matrix((w, (np.repeat(np.arange(nf), pcol.shape[1]), pcol.ravel())), shape=(nf, ncoarse)).tocsr()
        self.aP = abs(self.P)
        self.PT, self.aPT = self.P.T.tocsr(), self.aP.T.tocsr()

    def prolong(self, xc):
        return self.P @ np.asarray(xc, np.float64), self.aP @ np.abs(xc)

    def restrict(self, xf):
        return self.PT @ np.asarray(xf, np.float64), self.aPT @ np.abs(xf)

    def galerkin(self, A):
        """(P^T A P, |P|^T |A| |P|) for a scipy fine-level matrix A (3 x 3 blocks); A's values are replaced by their absolute values"""
        import scipy.sparse as sp
        P3, aP3 = sp.kron(self.P, sp.identity(3)).tocsr(), sp.kron(self.aP, sp.identity(3)).tocsr()
        rap = (P3.T @ (A @ P3)).tocsr()
        np.abs(A.data, out=A.data)
        return rap, (aP3.T @ (A @ aP3)).tocsr()


class Hierarchy:
    """Levels and transfers exported by a context after hot_build_mg."""

    def __init__(self, ctx, nlev):
        self.levels, self.transfers = [], []
        for l in range(nlev):
            col, val = ctx.matrix(l)
            self.levels.append(Level(col, val, ctx.level(l)["id2coord"]))
            del col, val
        for l in range(nlev - 1):
            pcol, pw = ctx.prolongation(l)
            self.transfers.append(Transfer(pcol, pw, self.levels[l + 1].n))

    def vcycle(self, x, times=1, levelscale=0, coarse_pcg=False):
        """The V-cycle (oracle/sim_matrix.hpp Sim::vcycle) with GS (kind 5) on every level below the top: times + l levelscale
        iterations down and up; on the top level GS too (coarseSolver = 5: (times + l levelscale) x 3 iterations) or, with coarse_pcg,
        PCG to its stopping rule against the restricted input (coarseSolver = 2).  Returns (out, m_out, K) where K adds up the
        constants of the chain (None with coarse_pcg: not a fixed operator)"""
        L = len(self.levels)
        its = lambda l: times + l * levelscale
        top = (lambda l: its(l) * 3) if L > 1 else its
        r, mr = [None] * L, [None] * L
        sol, msol = [None] * L, [None] * L
        r[0], mr[0] = np.asarray(x, np.float64), np.abs(np.asarray(x, np.float64))
        K = 0
        for l in range(L - 1):
            z = np.zeros((self.levels[l].n, 3))
            sol[l], r[l], msol[l], mr[l] = self.levels[l].gs(z, r[l], its(l), z, mr[l])
            r[l + 1], mr[l + 1] = self.transfers[l].PT @ r[l], self.transfers[l].aPT @ mr[l]
            K += k_gs(its(l)) + K_RESTRICT
        z = np.zeros((self.levels[L - 1].n, 3))
        if coarse_pcg:
            init = np.asarray(x, np.float64)  # the reference residual of the stopping rule: the restricted input
            for t in self.transfers:
                init = t.PT @ init
            sol[L - 1], r[L - 1], msol[L - 1], mr[L - 1] = self.levels[L - 1].pcg(z, r[L - 1], 10000, r0=init)[:4]
            K = None
        else:
            sol[L - 1], r[L - 1], msol[L - 1], mr[L - 1] = self.levels[L - 1].gs(z, r[L - 1], top(L - 1), z, mr[L - 1])
            K += k_gs(top(L - 1))
        for l in range(L - 2, -1, -1):
            d, md = self.transfers[l].P @ sol[l + 1], self.transfers[l].aP @ msol[l + 1]
            sol[l], msol[l] = sol[l] + d, msol[l] + md
            r[l], mr[l] = r[l] - self.levels[l].mul(d), mr[l] + self.levels[l].mul(md, self.levels[l].aW)
            sol[l], r[l], msol[l], mr[l] = self.levels[l].gs(sol[l], r[l], its(l), msol[l], mr[l])
            K = None if K is None else K + K_PROLONG + K_SPMV + 2 + k_gs(its(l))
        return sol[0], msol[0], K


def k_gs_invariant(iterations):
    """|r - (r0 - A u)| of kind 5 after `iterations`: per sweep the local residuals of the two substitutions (K_ROW each) and of the
    update r -= A du (K_SPMV), whichever way an implementation forms r (the true product, or L (h - du) of the two sweeps); relative to
    |r0| + |A| m_u, which bounds |A| |h| and |A| |du| of every sweep (m_du >= m_h since |D^-1| |D| >= I)"""
    return ((iterations + 1) >> 1) * (2 * K_ROW + K_SPMV + 4)


def k_update_invariant(iterations):
    """|r - (r0 - A u)| of kinds 0 / 1 / 2: per iteration the product dA u and the two updates"""
    return iterations * (K_SPMV + 4)


def sparse_ratio(got, ref, m, u):
    """largest |got - ref| / (u m) entrywise over sparse matrices; an entry with m = 0 must be exact (inf otherwise)"""
    d = abs(got - ref).tocsr()
    d.eliminate_zeros()
    if d.nnz == 0:
        return 0.0
    mm = m.tocsr()
    outside = d - d.multiply(mm > 0)
    outside.eliminate_zeros()
    if outside.nnz:
        return float("inf")
    q = d.multiply(mm.power(-1.0))
    return float(q.max()) / u


class Report:
    """Rows (operator, level, largest |got - ref| / (u m), K, normwise error); `check` asserts every ratio <= K"""

    def __init__(self, label, u):
        self.label, self.u, self.rows = label, u, []

    def add(self, op, level, got, ref, m, K, extra=""):
        self.rows.append((op, level, ratio(got, ref, m, self.u), K, normwise(got, ref), extra))

    def text(self):
        out = [f"[{self.label}] operator            level  max|err|/(u m)        K   ratio/K   normwise"]
        for op, l, q, K, nw, extra in self.rows:
            out.append(f"[{self.label}] {op:<20s} {l:>5}  {q:14.4g} {K:8d}  {q / K:8.2e}  {nw:9.2e} {extra}")
        return "\n".join(out)

    def check(self, normwise_tol=None):
        print(self.text())
        bad = [r for r in self.rows if not r[2] <= r[3]]
        assert not bad, ("componentwise bound exceeded", self.label, bad)
        if normwise_tol is not None:
            bad = [r for r in self.rows if not r[4] <= normwise_tol]
            assert not bad, ("normwise", self.label, bad)


def check_operators(ctx, ref, T, rep, nlev, gs_levels=None, smooth_its=(1, 2, 4), jacobi_levels=(0,), pcg_its=(), pcg_levels=(), galerkin=True, seed=0):
    """Every level operator of `ctx` (HIP library or oracle, after hot_build_mg) against the reference `ref` built from ctx's own
    exported levels; rows go to the Report `rep`."""
    rng = np.random.default_rng(seed)
    cast = lambda a: np.asarray(a, T).astype(np.float64)
    levels = ref.levels
    gs_levels = range(nlev) if gs_levels is None else gs_levels
    for l in range(nlev):
        L = levels[l]
        x = cast(rng.standard_normal((L.n, 3)))
        y, m = L.spmv(x)
        rep.add("spmv", l, ctx.spmv(l, x), y, m, K_SPMV)
        if l + 1 < nlev:
            tr = ref.transfers[l]
            y, m = tr.restrict(x)
            rep.add("restrict", l, ctx.restrict(l, x), y, m, K_RESTRICT)
            xc = cast(rng.standard_normal((levels[l + 1].n, 3)))
            y, m = tr.prolong(xc)
            rep.add("prolong", l, ctx.prolong(l, xc), y, m, K_PROLONG)
            if galerkin:
                A = L.dense()
                rap, mrap = tr.galerkin(A)
                del A
                A1 = levels[l + 1].dense()
                q = sparse_ratio(A1, rap, mrap, rep.u)
                nw = abs(A1 - rap).max() / abs(rap).max()
                rep.rows.append(("galerkin", l + 1, q, K_GALERKIN, nw, ""))
                del rap, mrap, A1

    def rhs(l):
        b = rng.standard_normal((levels[l].n, 3))
        return cast(ctx.project(b) if l == 0 else b)

    def invariant(l, r0, u_got, r_got, mu, K, name):
        L = levels[l]
        rep.add(name, l, r_got, r0 - L.mul(u_got), np.abs(r0) + L.mul(mu, L.aW), K)

    for l in gs_levels:
        for its in smooth_its:
            r0 = rhs(l)
            z = np.zeros_like(r0)
            ug, rg = ctx.smooth(l, 5, its, z, r0, tolerance=0.0)
            u, r, mu, mr = levels[l].gs(z, r0, its)
            rep.add(f"gs{its} u", l, ug, u, mu, k_gs(its))
            rep.add(f"gs{its} r", l, rg, r, mr, k_gs(its))
            invariant(l, r0, np.asarray(ug, np.float64), rg, mu, k_gs_invariant(its), f"gs{its} r0-Au")
    for l in jacobi_levels:
        for kind in (0, 1):
            its = 3
            r0 = rhs(l)
            z = np.zeros_like(r0)
            ug, rg = ctx.smooth(l, kind, its, z, r0, tolerance=0.0)
            u, r, mu, mr = levels[l].jacobi(z, r0, its, kind)
            rep.add(f"kind{kind}x{its} u", l, ug, u, mu, k_jacobi(its))
            rep.add(f"kind{kind}x{its} r", l, rg, r, mr, k_jacobi(its))
            invariant(l, r0, np.asarray(ug, np.float64), rg, mu, k_update_invariant(its), f"kind{kind}x{its} r0-Au")
    for l in pcg_levels:
        for its in pcg_its:
            r0 = rhs(l)
            z = np.zeros_like(r0)
            tiny = r0 * 2.0 ** -30  # the stopping rule's reference residual: z.r < z0.r0 / 4 never fires, `its` iterations run
            ug, rg = ctx.smooth(l, 2, its, z, r0, tolerance=0.0, initial_residual=np.asarray(tiny, T))
            u, r, mu, mr, cnt, _ = levels[l].pcg(z, r0, its, r0=tiny)
            assert cnt == its
            rep.add(f"pcg{its} u", l, ug, u, mu, k_pcg(its))
            rep.add(f"pcg{its} r", l, rg, r, mr, k_pcg(its))
            invariant(l, r0, np.asarray(ug, np.float64), rg, mu, k_update_invariant(its), f"pcg{its} r0-Au")
        # the reference's own stopping rule (r0 = r): the iteration count is part of the result
        r0 = rhs(l)
        z = np.zeros_like(r0)
        ug, rg = ctx.smooth(l, 2, 10, z, r0, tolerance=0.0)
        u, r, mu, mr, cnt, last = levels[l].pcg(z, r0, 10)
        if cnt == 10 or abs(last - 1) > 1e-6:  # (a stop decided within round-off of the threshold is not a fixed operator)
            rep.add(f"pcg-rule({cnt}) u", l, ug, u, mu, k_pcg(cnt))
