"""Trace of the host layer: every call ops.py / autograd.py make into libe2eft, argument for argument, over a fixed list of seeded cases.

    python scripts/host_trace.py run <package directory> <output directory> [name]      one package (any checkout's `diffusion-e2e-ft_amd/`) -> trace.json, tensors.pt
    python scripts/host_trace.py compare [--other-build] <output directory A> <output directory B> [report file]

`run` loads the package from the directory it is given (not the one next to this script), wraps every function of `_lib.SIGNATURES` on the loaded library and records
per call: the symbol, every field of a descriptor argument, every scalar, for each pointer null-or-not and its low four bits, the return value, and the kernel symbol
the library's dispatch picked (`ops._last_kernel()`) after each launch.  ops.TIMER is set, so (family, label, launches, flops, bytes, flops_nominal) of every timed
region are recorded too (no times).  The script sets the library options itself (persistent grid 0 and 8; for fp32 the split-plane route on and off), so a trace does
not depend on the environment it was started in.  The last leg is `__graft_entry__.smoke()` whole, with the peak of allocated bytes over it.

Every result that is kept is saved, and with it the GroupNorm statistics partials its producer attached (`_e2eft_gn`).

`compare` wants two traces to be the same JSON, every saved tensor bit-equal and the peaks equal: a refactor of the host layer that changes no library call.  With
--other-build the two libraries may carry different build ids (a refactor of the device code: same calls, same kernels picked, same bits); nothing else may differ.
Run the two `run`s as fresh processes (each initialises the GPU once)."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

REQUIRED = """e2eft_conv2d_fwd e2eft_conv2d_fwd_gnstats e2eft_conv2d_fwd_splitk e2eft_conv2d_fwd_normed e2eft_conv2d_fwd_f32split e2eft_upconv2x_fwd
e2eft_upconv2x_fwd_f32split e2eft_gemm e2eft_gemm_gnstats e2eft_gemm_f32split e2eft_groupnorm_fwd_pre e2eft_groupnorm_fwd_stats e2eft_groupnorm_fwd_split
e2eft_groupnorm_bwd_add e2eft_conv2d_dgrad e2eft_conv2d_wgrad e2eft_conv2d_im2col_t e2eft_transpose e2eft_colsum e2eft_f32_split2 e2eft_f32_split2_cat
e2eft_f32_split2_cols e2eft_f32_split_weight e2eft_f32_split_wgrad_finish""".split()


def load_package(pkg_dir):
    """what the import shim at the repository root does, for the directory given"""
    import types
    pkg_dir = os.path.abspath(pkg_dir)
    mod = types.ModuleType("diffusion_e2e_ft_amd")
    mod.__path__ = [pkg_dir]
    mod.__file__ = os.path.join(pkg_dir, "__init__.py")
    sys.modules["diffusion_e2e_ft_amd"] = mod
    with open(mod.__file__) as f:
        exec(compile(f.read(), mod.__file__, "exec"), mod.__dict__)
    return mod


class Tracer:
    def __init__(self, _lib, ops):
        self.calls, self.ops = [], ops
        lib = _lib.load()
        for name, (res, argtypes) in _lib.SIGNATURES.items():
            setattr(lib, name, self._wrap(name, getattr(lib, name), res, argtypes))

    @staticmethod
    def _arg(a, ty):
        if ty is C.c_void_p:
            v = a.value if isinstance(a, C.c_void_p) else a
            return ["ptr", 0 if not v else 1, (v or 0) & 15]
        if isinstance(ty, type) and issubclass(ty, C._Pointer):
            if a is None:
                return ["ref", None]
            obj = a._obj                                                   # C.byref(struct or scalar)
            if isinstance(obj, C.Structure):
                return [type(obj).__name__, {f: (list(getattr(obj, f)) if isinstance(getattr(obj, f), C.Array) else getattr(obj, f)) for f, _ in obj._fields_}]
            return ["ref", obj]                                            # an out scalar: its value is read after the call
        return a.value if hasattr(a, "value") else a

    def _wrap(self, name, fn, res, argtypes):
        query = name.endswith(("_supported", "_workspace_bytes", "_offset")) or name in ("e2eft_version", "e2eft_last_error", "e2eft_build_id", "e2eft_set_option", "e2eft_get_option")

        def call(*args):
            rec = [self._arg(a, t) for a, t in zip(args, argtypes)]
            ret = fn(*args)
            for r in rec:                                                  # out scalars (slab rows, split counts)
                if isinstance(r, list) and r[0] == "ref" and r[1] is not None:
                    r[1] = r[1].value
            entry = {"fn": name, "args": rec, "ret": ret.decode() if isinstance(ret, bytes) else ret}
            if not query:
                entry["kernel"] = self.ops._last_kernel()
            self.calls.append(entry)
            return ret

        return call


def run(pkg_dir, out_dir, name=None):
    import torch
    load_package(pkg_dir)
    from diffusion_e2e_ft_amd import _lib, ops, autograd as F
    os.makedirs(out_dir, exist_ok=True)
    _lib.load()
    build_id = _lib.build_id()
    tr = Tracer(_lib, ops)
    ops.TIMER = ops.KernelTimer()
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(20240)
    saved, ncases = [], [0]

    def rnd(*shape, dt=torch.float16, grad=False, scale=1.0):
        return (torch.randn(*shape, generator=gen) * scale).to(dev, dt).requires_grad_(grad)

    def keep(*ts):
        for t in ts:
            if isinstance(t, (tuple, list)):
                keep(*t)
            elif t is not None:
                saved.append(t.detach().float().cpu() if t.dtype == torch.bfloat16 else t.detach().cpu())
                st = getattr(t, "_e2eft_gn", None)                         # the statistics partials the producer attached: [images, nslabs, C, 3] fp32
                if st is not None:
                    saved.append(st.partial.detach().cpu())

    def conv_mod(cin, cout, k, stride, dt, frozen=False):
        m = torch.nn.Conv2d(cin, cout, k, stride, k // 2)
        with torch.no_grad():
            m.weight.copy_(torch.randn(m.weight.shape, generator=gen) * (cin * k * k) ** -0.5)
            m.bias.copy_(torch.randn(cout, generator=gen) * 0.1)
        return m.to(dev, dt).requires_grad_(not frozen)

    def norm_mod(c, dt):
        m = torch.nn.GroupNorm(32 if c % 32 == 0 else 4, c)
        with torch.no_grad():
            m.weight.copy_(1.0 + 0.1 * torch.randn(c, generator=gen))
            m.bias.copy_(0.1 * torch.randn(c, generator=gen))
        return m.to(dev, dt)

    def backward(y, *leaves):
        ys = [t for t in (y if isinstance(y, (tuple, list)) else (y,)) if t.requires_grad]
        torch.autograd.backward(ys, [rnd(*t.shape, dt=t.dtype) for t in ys])
        keep([p.grad for p in leaves if p is not None])

    def conv_case(dt, cin, cout, k=3, stride=1, pad=None, B=1, H=64, W=64, cin2=0, norm=False, residual=False, rowadd=False, gn_stats=False, up=False, producer=False,
                  phase=True):
        """forward without a gradient (the fused-norm / split-plane routes), then forward + backward through autograd.py"""
        ncases[0] += 1
        conv, gn = conv_mod(cin + cin2, cout, k, stride, dt), norm_mod(cin + cin2, dt) if norm else None
        up_to = (2 * H, 2 * W) if up else None
        ops.UPCONV_PHASES_ENABLED = phase
        for grad in (False, True):
            x = rnd(B, H, W, cin, dt=dt, grad=grad)
            if producer:      # x comes from a convolution that leaves GroupNorm statistics on it
                x = F.conv(conv_mod(cin, cin, 3, 1, dt), x, gn_stats=True)
            x2 = rnd(B, H, W, cin2, dt=dt, grad=grad) if cin2 else None
            hl, wl = up_to or (H, W)
            pd = pad or (k // 2,) * 4
            ho, wo = (hl + pd[0] + pd[1] - k) // stride + 1, (wl + pd[2] + pd[3] - k) // stride + 1
            res = rnd(B, ho, wo, cout, dt=dt, grad=grad) if residual else None
            row = rnd(B, cout, dt=dt, grad=grad) if rowadd else None
            with torch.set_grad_enabled(grad):
                y = F.conv(conv, x, x2=x2, up_to=up_to, rowadd=row, residual=res, pad=pad, gn_stats=gn_stats, norm=(gn, True) if norm else None, alpha=0.5 if residual else 1.0)
            keep(y)
            if grad:
                backward(y, conv.weight, conv.bias, x if x.is_leaf else None, x2, res, row, gn.weight if norm else None, gn.bias if norm else None)
                for p in list(conv.parameters()) + (list(gn.parameters()) if norm else []):
                    p.grad = None
        ops.UPCONV_PHASES_ENABLED = True

    def conv_cases(dt):
        for (ci, co) in ((64, 128), (128, 64)):
            conv_case(dt, ci, co)
            conv_case(dt, ci, co, norm=True)
            conv_case(dt, ci, co, norm=True, producer=True)
            conv_case(dt, ci, co, residual=True)
            conv_case(dt, ci, co, rowadd=True)
            conv_case(dt, ci, co, gn_stats=True)
            conv_case(dt, ci, co, norm=True, residual=True, rowadd=True, gn_stats=True)
        for kw in (dict(), dict(norm=True), dict(residual=True), dict(rowadd=True), dict(gn_stats=True)):
            conv_case(dt, 64, 64, cin2=64, **kw)
        conv_case(dt, 64, 64, k=1)
        conv_case(dt, 64, 64, stride=2, pad=(0, 1, 0, 1))
        conv_case(dt, 64, 64, stride=2, pad=(1, 1, 1, 1))
        conv_case(dt, 8, 64)
        conv_case(dt, 64, 4)
        conv_case(dt, 64, 4, norm=True)
        conv_case(dt, 1280, 1280, H=8, W=8)
        conv_case(dt, 1280, 1280, H=8, W=8, norm=True)
        for ci in (64, 128):
            conv_case(dt, ci, 64, B=4, H=32, W=32, up=True)      # (four images: the phases need two tiles per workgroup of the 8-workgroup grid)
            conv_case(dt, ci, 64, B=4, H=32, W=32, up=True, phase=False)
        # the norm's own pass inside ops.conv2d (two sources; fusion switched off), into a caller's buffer
        ncases[0] += 1
        conv, gn = conv_mod(128, 64, 3, 1, dt), norm_mod(128, dt)
        w, nrm = F.packed_conv_weight(conv, dt), (gn.weight.detach(), gn.bias.detach(), gn.num_groups, gn.eps, True)
        x, x2, out = rnd(1, 64, 64, 64, dt=dt), rnd(1, 64, 64, 64, dt=dt), torch.empty((1, 64, 64, 64), dtype=dt, device=dev)
        with torch.no_grad():
            keep(ops.conv2d(x, w, conv.bias.detach(), 64, 3, 3, 1, (1, 1, 1, 1), x2=x2, norm=nrm, out=out, gn_stats=True))
            ops.NORM_FUSION_ENABLED = False
            keep(ops.conv2d(torch.cat((x, x2), -1), w, conv.bias.detach(), 64, 3, 3, 1, (1, 1, 1, 1), norm=nrm))
            ops.NORM_FUSION_ENABLED = True
        # weight gradient on the transpose + im2col_t + split-K GEMM path
        ops.WGRAD_DIRECT = False
        conv_case(dt, 64, 128)
        conv_case(dt, 64, 64, cin2=64)
        ops.WGRAD_DIRECT = True

    def linear_cases(dt):
        for (M, K, N) in ((512, 64, 64), (256, 64, 192), (512, 320, 192), (256, 320, 64)):
            for nw, rows in ((1, 0), (1, 128), (3, 0)):
                ncases[0] += 1
                owner = torch.nn.Module()
                ws = [torch.nn.Parameter(rnd(N, K, dt=dt, scale=K ** -0.5)) for _ in range(nw)]
                b = torch.nn.Parameter(rnd(N * nw, dt=dt, scale=0.1))
                for grad in (False, True):
                    x, res = rnd(2, M // 2, K, dt=dt, grad=grad), rnd(2, M // 2, N * nw, dt=dt, grad=grad)
                    with torch.set_grad_enabled(grad):
                        y = F.linear(x, tuple(ws), b, residual=res, owner=owner, name="w", gn_rows_per_image=rows)
                    keep(y)
                    if grad:
                        backward(y, x, res, b, *ws)

    def groupnorm_cases(dt):
        for c2 in (0, 64):
            for split in (False, True):
                for producer in (False, True):
                    ncases[0] += 1
                    gn = norm_mod(64 + c2, dt)
                    for grad in (False, True):
                        x = rnd(1, 64, 64, 64, dt=dt, grad=grad)
                        if producer:
                            x = F.conv(conv_mod(64, 64, 3, 1, dt), x, gn_stats=True)
                        x2 = rnd(1, 64, 64, c2, dt=dt, grad=grad) if c2 else None
                        with torch.set_grad_enabled(grad):
                            y = F.groupnorm(x, gn.weight, gn.bias, gn.num_groups, gn.eps, silu=True, x2=x2, split=split)
                        keep(y)
                        if grad:
                            backward(y, gn.weight, gn.bias, x if x.is_leaf else None, x2)
                            gn.weight.grad = gn.bias.grad = None

    def norm_conv_split_cases(must_take):
        for (ci, co, res, split) in ((64, 128, False, False), (128, 64, False, True), (64, 64, True, True)):
            ncases[0] += 1
            conv, gn = conv_mod(ci, co, 3, 1, torch.float32, frozen=True), norm_mod(ci, torch.float32)
            x = F.conv(conv_mod(ci, ci, 3, 1, torch.float32, frozen=True), rnd(1, 64, 64, ci, dt=torch.float32, grad=True), gn_stats=True)
            r = rnd(1, 64, 64, co, dt=torch.float32, grad=True) if res else None
            y = F.norm_conv_split(conv, gn, x, True, residual=r, split=split)
            if y is None:      # (at the device's own grid these shapes are too small for the persistent kernels: the route declines, its queries are in the trace)
                assert not must_take, "norm_conv_split declined the case"
                continue
            keep(y)
            backward(y, gn.weight, gn.bias, r)

    legs = []
    grid0, split0 = _lib.load().e2eft_get_option(_lib.OPT_PERSISTENT_GRID), _lib.load().e2eft_get_option(_lib.OPT_F32_SPLIT)
    for grid in (0, 8):
        _lib.set_option(_lib.OPT_PERSISTENT_GRID, grid)
        legs.append(("fp16 grid %d" % grid, len(tr.calls)))
        conv_cases(torch.float16)
        linear_cases(torch.float16)
        groupnorm_cases(torch.float16)
        for split in (1, 0):
            _lib.set_option(_lib.OPT_F32_SPLIT, split)
            legs.append(("fp32 grid %d split %d" % (grid, split), len(tr.calls)))
            conv_cases(torch.float32)
            linear_cases(torch.float32)
            groupnorm_cases(torch.float32)
            if split:
                norm_conv_split_cases(must_take=grid == 8)
    torch.cuda.synchronize()
    _lib.set_option(_lib.OPT_PERSISTENT_GRID, grid0)
    _lib.set_option(_lib.OPT_F32_SPLIT, split0)
    legs.append(("smoke", len(tr.calls)))
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    sys.path.insert(0, ROOT)
    import __graft_entry__
    __graft_entry__.smoke()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    timer = [[fam, r[4], r[5], r[2], r[3], r[6]] for fam, lst in ops.TIMER.rec.items() for r in lst]
    seen = {c["fn"] for c in tr.calls}
    missing = [s for s in REQUIRED if s not in seen]
    with open(os.path.join(out_dir, "trace.json"), "w") as f:
        json.dump({"legs": legs, "cases": ncases[0], "calls": tr.calls, "timer": timer, "smoke_peak_allocated": peak, "allocated_before_smoke": base}, f, indent=0)
    with open(os.path.join(out_dir, "meta.json"), "w") as f:      # what may differ between two checkouts
        json.dump({"build_id": build_id, "package": name or pkg_dir, "missing": missing}, f)
    torch.save(saved, os.path.join(out_dir, "tensors.pt"))
    print("host_trace: %d cases, %d library calls, %d timed regions, %d tensors, smoke peak %d bytes, build id %s" % (ncases[0], len(tr.calls), len(timer), len(saved), peak, build_id))
    if missing:
        print("host_trace: the case list does not reach: %s" % " ".join(missing))
        return 1
    return 0


def compare(a_dir, b_dir, report=None, other_build=False):
    import torch
    lines, bad = [], 0
    ja, jb = (json.load(open(os.path.join(d, "trace.json"))) for d in (a_dir, b_dir))
    ma, mb = (json.load(open(os.path.join(d, "meta.json"))) for d in (a_dir, b_dir))
    lines.append("A: %s build id %s" % (ma["package"], ma["build_id"]))
    lines.append("B: %s build id %s" % (mb["package"], mb["build_id"]))
    lines.append("cases: %d / %d, library calls: %d / %d, timed regions: %d / %d" % (ja["cases"], jb["cases"], len(ja["calls"]), len(jb["calls"]), len(ja["timer"]), len(jb["timer"])))
    for k in ("calls", "timer"):
        for i, (x, y) in enumerate(zip(ja[k], jb[k])):
            if x != y:
                bad += 1
                lines.append("%s[%d] differ:\n  A %s\n  B %s" % (k, i, json.dumps(x), json.dumps(y)))
                break                                                      # the first difference of a stream; what follows it usually follows from it
        if len(ja[k]) != len(jb[k]):
            bad += 1
            lines.append("%s: %d entries against %d" % (k, len(ja[k]), len(jb[k])))
    for k in ("legs", "cases", "smoke_peak_allocated", "allocated_before_smoke"):
        if ja[k] != jb[k]:
            bad += 1
            lines.append("%s: %s against %s" % (k, ja[k], jb[k]))
    lines.append("smoke peak allocated bytes: %d / %d" % (ja["smoke_peak_allocated"], jb["smoke_peak_allocated"]))
    ta, tb = (torch.load(os.path.join(d, "tensors.pt")) for d in (a_dir, b_dir))
    ints = {2: torch.int16, 4: torch.int32, 8: torch.int64, 1: torch.uint8}
    neq = [i for i, (x, y) in enumerate(zip(ta, tb)) if x.shape != y.shape or x.dtype != y.dtype
           or not torch.equal(x.contiguous().view(ints[x.element_size()]), y.contiguous().view(ints[y.element_size()]))]      # bit patterns: a NaN equals itself
    if neq or len(ta) != len(tb):
        bad += 1
    lines.append("tensors: %d / %d saved, %d not bit-equal%s" % (len(ta), len(tb), len(neq), (" (first: #%d)" % neq[0]) if neq else ""))
    if ma["build_id"] != mb["build_id"]:
        if other_build:
            lines.append("the two libraries differ, as expected (--other-build)")
        else:
            bad += 1
            lines.append("the two libraries differ")
    lines.append("differences: %d%s" % (bad, "" if bad else " (the two sides make the same library calls, pick the same kernels and compute the same bits)"))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if report:
        with open(report, "w") as f:
            f.write(text)
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) >= 4 and sys.argv[1] == "run":
        sys.exit(run(*sys.argv[2:5]))
    if len(sys.argv) >= 4 and sys.argv[1] == "compare":
        args = [a for a in sys.argv[2:] if a != "--other-build"]
        sys.exit(compare(args[0], args[1], args[2] if len(args) > 2 else None, other_build="--other-build" in sys.argv))
    sys.exit(__doc__)
