"""Float64 NumPy restatement of L-BFGS-B 3.0 on unbounded problems (nbd = 0 everywhere) as scipy's minimize(method='L-BFGS-B') drives
it -- the state machine the device step kernel (csrc/lbfgs.hip) implements, written from the published algorithm:

  * reverse communication: `iterate(f, g)` consumes f and g at the last requested point and returns (task, x_next); task codes are scipy's
    (task[0], task[1]) pairs (_lbfgsb_py.py status_messages / task_messages): (3, 0) FG, (4, 401) / (4, 402) CONVERGENCE,
    (5, 504) / (5, 502) STOP, (8, 0) ABNORMAL;
  * direction: with no stored pair the Cauchy point at theta = 1, z = x + (-g); otherwise z = x + (-H g), H the L-BFGS inverse over the
    last m pairs with H0 = I / theta, theta = y.y / s.y of the newest pair (two-loop recursion: the same vector as L-BFGS-B's compact
    form); d = z - x in both cases, as mainlb forms it;
  * line search: lnsrlb + MINPACK-2 dcsrch / dcstep (ftol 1e-3, gtol 0.9, xtol 0.1, stpmin 0, stpmax 1e10), first step min(1/|d|, 1e10)
    at iteration 0 and 1 afterwards, the trial x = z when stp == 1 and stp * d + t otherwise; a WARNING outcome is accepted;
  * line-search failure (g.d >= 0 at the start, or the (maxls + 1)-th trial requested): x, g, f back to the start of the search; ABNORMAL
    with no stored pair, otherwise the memory is dropped and the search restarts from the Cauchy direction;
  * at NEW_X, the wrapper's counters first (nit += 1; nit >= maxiter -> STOP 504, else nfev > maxfun -> STOP 502), then setulb's tests on
    its next entry (max|g| <= gtol -> 401; fold - f <= (ftol / eps) * eps * max(|fold|, |f|, 1) -> 402), then the pair update, skipped when
    s.y <= eps * (-g_old.d * stp);
  * nfev counts evaluations as scipy's ScalarFunction does: a requested point bitwise equal to the last evaluated one is not evaluated again.

`minimize(fun_and_grad, x0, ...)` drives it the way scipy's wrapper does and returns fun, x, nit, nfev, status, message and the list of
evaluated points."""
import numpy as np

EPS = np.finfo(np.float64).eps
STATUS = {0: "START", 1: "NEW_X", 2: "RESTART", 3: "FG", 4: "CONVERGENCE", 5: "STOP", 6: "WARNING", 7: "ERROR", 8: "ABNORMAL"}
TASK = {0: "", 401: "NORM OF PROJECTED GRADIENT <= PGTOL", 402: "RELATIVE REDUCTION OF F <= FACTR*EPSMCH",
        502: "TOTAL NO. OF F,G EVALUATIONS EXCEEDS LIMIT", 504: "TOTAL NO. OF ITERATIONS REACHED LIMIT"}
FG, CONV_PG, CONV_F, STOP_ITER, STOP_FUN, ABNORMAL = (3, 0), (4, 401), (4, 402), (5, 504), (5, 502), (8, 0)
DEFAULTS = dict(m=10, maxls=20, maxiter=15000, maxfun=15000, ftol=2.220446049250313e-09, gtol=1e-5)
LS_FTOL, LS_GTOL, LS_XTOL, STPMAX = 1e-3, 0.9, 0.1, 1e10


def message(task):
    return STATUS[task[0]] + ": " + TASK.get(task[1], "")


def status_of(task, nit, nfev, maxiter, maxfun):
    """scipy's warnflag: 0 converged, 1 a limit, 2 anything else."""
    if task[0] == 4:
        return 0
    return 1 if (nfev > maxfun or nit >= maxiter) else 2


def dcstep(stx, fx, dx, sty, fy, dy, stp, fp, dp, brackt, stpmin, stpmax):
    """MINPACK-2 dcstep (More & Thuente): the safeguarded step; returns (stx, fx, dx, sty, fy, dy, stp, brackt)."""
    sgnd = dp * (dx / abs(dx))
    if fp > fx:
        theta = 3.0 * (fx - fp) / (stp - stx) + dx + dp
        s = max(abs(theta), abs(dx), abs(dp))
        gamma = s * np.sqrt((theta / s) * (theta / s) - (dx / s) * (dp / s))
        if stp < stx:
            gamma = -gamma
        p = (gamma - dx) + theta
        q = ((gamma - dx) + gamma) + dp
        r = p / q
        stpc = stx + r * (stp - stx)
        stpq = stx + ((dx / ((fx - fp) / (stp - stx) + dx)) / 2.0) * (stp - stx)
        stpf = stpc if abs(stpc - stx) < abs(stpq - stx) else stpc + (stpq - stpc) / 2.0
        brackt = True
    elif sgnd < 0.0:
        theta = 3.0 * (fx - fp) / (stp - stx) + dx + dp
        s = max(abs(theta), abs(dx), abs(dp))
        gamma = s * np.sqrt((theta / s) * (theta / s) - (dx / s) * (dp / s))
        if stp > stx:
            gamma = -gamma
        p = (gamma - dp) + theta
        q = ((gamma - dp) + gamma) + dx
        r = p / q
        stpc = stp + r * (stx - stp)
        stpq = stp + (dp / (dp - dx)) * (stx - stp)
        stpf = stpc if abs(stpc - stp) > abs(stpq - stp) else stpq
        brackt = True
    elif abs(dp) < abs(dx):
        theta = 3.0 * (fx - fp) / (stp - stx) + dx + dp
        s = max(abs(theta), abs(dx), abs(dp))
        gamma = s * np.sqrt(max(0.0, (theta / s) * (theta / s) - (dx / s) * (dp / s)))
        if stp > stx:
            gamma = -gamma
        p = (gamma - dp) + theta
        q = (gamma + (dx - dp)) + gamma
        r = p / q
        if r < 0.0 and gamma != 0.0:
            stpc = stp + r * (stx - stp)
        elif stp > stx:
            stpc = stpmax
        else:
            stpc = stpmin
        stpq = stp + (dp / (dp - dx)) * (stx - stp)
        if brackt:
            stpf = stpc if abs(stpc - stp) < abs(stpq - stp) else stpq
            if stp > stx:
                stpf = min(stp + 0.66 * (sty - stp), stpf)
            else:
                stpf = max(stp + 0.66 * (sty - stp), stpf)
        else:
            stpf = stpc if abs(stpc - stp) > abs(stpq - stp) else stpq
            stpf = min(stpmax, stpf)
            stpf = max(stpmin, stpf)
    else:
        if brackt:
            theta = 3.0 * (fp - fy) / (sty - stp) + dy + dp
            s = max(abs(theta), abs(dy), abs(dp))
            gamma = s * np.sqrt((theta / s) * (theta / s) - (dy / s) * (dp / s))
            if stp > sty:
                gamma = -gamma
            p = (gamma - dp) + theta
            q = ((gamma - dp) + gamma) + dy
            r = p / q
            stpc = stp + r * (sty - stp)
            stpf = stpc
        elif stp > stx:
            stpf = stpmax
        else:
            stpf = stpmin
    if fp > fx:
        sty, fy, dy = stp, fp, dp
    else:
        if sgnd < 0.0:
            sty, fy, dy = stx, fx, dx
        stx, fx, dx = stp, fp, dp
    return stx, fx, dx, sty, fy, dy, stpf, brackt


class Dcsrch(object):
    """MINPACK-2 dcsrch with stpmin = 0: start(f, g, stp) opens a search, step(f, g) returns 'FG', 'CONV' or 'WARN' and moves self.stp."""

    def start(self, f, g, stp):
        self.stp, self.brackt, self.stage = stp, False, 1
        self.finit, self.ginit = f, g
        self.gtest = LS_FTOL * g
        self.width = STPMAX - 0.0
        self.width1 = self.width / 0.5
        self.stx, self.fx, self.gx = 0.0, f, g
        self.sty, self.fy, self.gy = 0.0, f, g
        self.stmin, self.stmax = 0.0, stp + 4.0 * stp

    def step(self, f, g):
        stp, gtest = self.stp, self.gtest
        ftest = self.finit + stp * gtest
        if self.stage == 1 and f <= ftest and g >= 0.0:
            self.stage = 2
        task = 'FG'
        if self.brackt and (stp <= self.stmin or stp >= self.stmax):
            task = 'WARN'
        if self.brackt and self.stmax - self.stmin <= LS_XTOL * self.stmax:
            task = 'WARN'
        if stp == STPMAX and f <= ftest and g <= gtest:
            task = 'WARN'
        if stp == 0.0 and (f > ftest or g >= gtest):
            task = 'WARN'
        if f <= ftest and abs(g) <= LS_GTOL * (-self.ginit):
            task = 'CONV'
        if task != 'FG':
            return task
        if self.stage == 1 and f <= self.fx and f > ftest:
            fm, fxm, fym = f - stp * gtest, self.fx - self.stx * gtest, self.fy - self.sty * gtest
            gm, gxm, gym = g - gtest, self.gx - gtest, self.gy - gtest
            self.stx, fxm, gxm, self.sty, fym, gym, stp, self.brackt = dcstep(
                self.stx, fxm, gxm, self.sty, fym, gym, stp, fm, gm, self.brackt, self.stmin, self.stmax)
            self.fx, self.fy = fxm + self.stx * gtest, fym + self.sty * gtest
            self.gx, self.gy = gxm + gtest, gym + gtest
        else:
            self.stx, self.fx, self.gx, self.sty, self.fy, self.gy, stp, self.brackt = dcstep(
                self.stx, self.fx, self.gx, self.sty, self.fy, self.gy, stp, f, g, self.brackt, self.stmin, self.stmax)
        if self.brackt:
            if abs(self.sty - self.stx) >= 0.66 * self.width1:
                stp = self.stx + 0.5 * (self.sty - self.stx)
            self.width1 = self.width
            self.width = abs(self.sty - self.stx)
            self.stmin, self.stmax = min(self.stx, self.sty), max(self.stx, self.sty)
        else:
            self.stmin = stp + 1.1 * (stp - self.stx)
            self.stmax = stp + 4.0 * (stp - self.stx)
        stp = min(max(stp, 0.0), STPMAX)
        if (self.brackt and (stp <= self.stmin or stp >= self.stmax)) or (self.brackt and self.stmax - self.stmin <= LS_XTOL * self.stmax):
            stp = self.stx
        self.stp = stp
        return 'FG'


class LbfgsState(object):
    """The reverse-communication core: LbfgsState(x0, **opts); then task, x = iterate(f, g) until task != FG (x: the point to evaluate
    next, or the final iterate)."""

    def __init__(self, x0, m=10, maxls=20, maxiter=15000, maxfun=15000, ftol=DEFAULTS['ftol'], gtol=1e-5):
        self.m, self.maxls, self.maxiter, self.maxfun = int(m), int(maxls), int(maxiter), int(maxfun)
        self.ftol, self.gtol = float(ftol), float(gtol)
        self.tol = (self.ftol / EPS) * EPS              # scipy passes factr = ftol / eps, setulb tests against factr * epsmch
        self.x = np.array(x0, dtype=np.float64)
        self.n = self.x.size
        self.S, self.Y, self.sy = [], [], []            # oldest first, at most m pairs
        self.theta = 1.0
        self.nit = self.nfev = 0
        self.phase = 'start'
        self.task = FG
        self.x_eval = None                              # the last point handed out for evaluation (the evaluation cache's key)
        self.ls = Dcsrch()

    # ---- pieces of mainlb
    def _direction(self):
        if not self.S:
            self.z = self.x + (-self.g)
        else:
            q = -self.g
            alpha = [0.0] * len(self.S)
            for i in range(len(self.S) - 1, -1, -1):
                alpha[i] = np.dot(self.S[i], q) / self.sy[i]
                q = q - alpha[i] * self.Y[i]
            r = q / self.theta
            for i in range(len(self.S)):
                beta = np.dot(self.Y[i], r) / self.sy[i]
                r = r + self.S[i] * (alpha[i] - beta)
            self.z = self.x + r
        self.d = self.z - self.x

    def _trial(self):
        """the next line-search point (lnsrlb: ifun += 1, iback = ifun - 1); False when that is the (maxls + 1)-th trial."""
        self.ifun += 1
        self.iback = self.ifun - 1
        if self.iback >= self.maxls:
            return False
        self.x = self.z.copy() if self.ls.stp == 1.0 else self.ls.stp * self.d + self.t
        return True

    def _search_start(self):
        """222 -> 666: direction, then lnsrlb's first entry; True when a trial point is set, False on a line-search failure."""
        self._direction()
        dnorm = np.sqrt(np.dot(self.d, self.d))
        stp = min(1.0 / dnorm, STPMAX) if self.nit == 0 else 1.0
        self.t, self.r, self.fold = self.x.copy(), self.g.copy(), self.f
        self.ifun = self.iback = 0
        self.gd = self.gdold = np.dot(self.g, self.d)
        if self.gd >= 0.0:
            return False
        self.ls.start(self.f, self.gd, stp)
        return self._trial()

    def _fail(self):
        """the restore of mainlb after a failed search: True to restart, False when the run ends ABNORMAL."""
        self.x, self.g, self.f = self.t.copy(), self.r.copy(), self.fold
        if not self.S:
            return False
        self.S, self.Y, self.sy, self.theta = [], [], [], 1.0
        return True

    def _search(self):
        """a search from the current iterate (restarting once after a failure at col > 0)."""
        while not self._search_start():
            if not self._fail():
                return self._finish(ABNORMAL)
        return self._emit()

    def _emit(self):
        self.task = FG
        return self.task, self.x

    def _finish(self, task):
        self.task = task
        self.phase = 'done'
        return self.task, self.x

    def iterate(self, f, g):
        if self.phase == 'done':
            return self.task, self.x
        self.f, self.g = float(f), np.array(g, dtype=np.float64)
        if self.x_eval is None or not np.array_equal(self.x, self.x_eval):
            self.nfev += 1
        self.x_eval = self.x.copy()
        if self.phase == 'start':
            self.phase = 'search'
            if np.max(np.abs(self.g)) <= self.gtol:
                return self._finish(CONV_PG)
            return self._search()
        # 556 of lnsrlb: the next dcsrch step
        self.gd = np.dot(self.g, self.d)
        if self.ls.step(self.f, self.gd) == 'FG':
            if self._trial():
                return self._emit()
            if not self._fail():
                return self._finish(ABNORMAL)
            return self._search()
        # NEW_X: the wrapper's counters, then setulb's tests at 777, then the pair
        self.nit += 1
        if self.nit >= self.maxiter:
            return self._finish(STOP_ITER)
        if self.nfev > self.maxfun:
            return self._finish(STOP_FUN)
        if np.max(np.abs(self.g)) <= self.gtol:
            return self._finish(CONV_PG)
        if self.fold - self.f <= self.tol * max(abs(self.fold), abs(self.f), 1.0):
            return self._finish(CONV_F)
        y = self.g - self.r
        stp = self.ls.stp
        if stp == 1.0:
            dr, ddum, s = self.gd - self.gdold, -self.gdold, self.d
        else:
            dr, ddum, s = (self.gd - self.gdold) * stp, -self.gdold * stp, stp * self.d
        if not dr <= EPS * ddum:
            if len(self.S) == self.m:
                self.S.pop(0); self.Y.pop(0); self.sy.pop(0)
            self.S.append(s.copy()); self.Y.append(y); self.sy.append(dr)
            self.theta = np.dot(y, y) / dr
        return self._search()


class Result(dict):
    __getattr__ = dict.__getitem__


def minimize(fun_and_grad, x0, **opts):
    """scipy.optimize.minimize(fun_and_grad, x0, jac=True, method='L-BFGS-B', options=...) on an unbounded problem, by the restatement;
    opts: m (maxcor), maxls, maxiter, maxfun, ftol, gtol.  `xs` lists every evaluated point; `x_final` is the last accepted iterate."""
    o = dict(DEFAULTS); o.update(opts)
    st = LbfgsState(x0, **o)
    xs, task, x = [], FG, st.x
    fun = None
    while task == FG:
        if st.x_eval is None or not np.array_equal(x, st.x_eval):
            xs.append(x.copy())
            fun, g = fun_and_grad(x.copy())
        task, x = st.iterate(fun, g)
    return Result(fun=float(fun), x=x.copy(), nit=st.nit, nfev=st.nfev, task=task, message=message(task), xs=xs,
                  status=status_of(task, st.nit, st.nfev, o['maxiter'], o['maxfun']))
