"""The scratch contract rows of the variational bound's entries (csrc/vlb_eval.hip), in the form of tests/scratch_rows.py: one row per
launch that consumes sr3_vlb_terms_partials_bytes.  tests/test_vlb_scratch_contract_cpu.py runs them through the host checks of
tests/test_scratch_contract_cpu.py, tests/test_gpu_vlb_eval.py through the guarded-buffer check of tests/test_gpu_scratch_contract.py."""
import torch

from scratch_rows import Row


def vlb_terms_row(prior):
    def build():
        from test_learned_var_cpu import loss_inputs, _ac
        import vlb_eval_ref as V
        d = loss_inputs()
        B, C2, H, W = d['out'].shape
        Cc, HW = C2 // 2, H * W
        abar = float(_ac()[-1])
        rows = torch.arange(B, dtype=torch.int32)

        def call(lib, P, scratch, nbytes, stream):
            if prior:
                sa, var, lv = V.prior_scalars(abar)
                return lib.sr3_prior_bpd_f32(P['hr'], B, Cc * HW, sa, var, lv, P['vb'], scratch, nbytes, stream)
            return lib.sr3_vlb_terms_f32(P['hr'], P['xt'], P['out'], C2, P['scal32'], B, P['rows'], None, 0, 0, B, Cc, HW, P['vb'], P['mse'], scratch,
                                         nbytes, stream)

        def check(got):
            # tests/test_gpu_vlb_eval.py's float64 references and its rule for the bound: 4 x the worst element error of the fp32 NumPy
            # restatement in the image, the conditioning of the last-step logs, one rounding of the result
            if prior:
                p64 = V.prior64(d['hr'], abar)
                ref = V.per_image(p64)
                tol = 4.0 * (torch.from_numpy(V.prior32(d['hr'].numpy(), abar)).double() - p64).abs().reshape(B, -1).max(1).values + 2.0 ** -24 * ref.abs()
                assert bool(((got['vb'].double() - ref).abs() <= tol).all())
                return
            s64 = d['scal32'].double().numpy()
            v64, m64 = V.terms64(d['hr'], d['xt'], d['out'], s64, 0, False)
            v32, m32 = V.terms32(d['hr'].numpy(), d['xt'].numpy(), d['out'].numpy(), d['scal32'].numpy(), 0, False)
            for name, r64, r32, cond in (('vb', v64, v32, V.nll_cond_per_image(d['hr'], d['xt'], d['out'], s64, 0, False)), ('mse', m64, m32, 0.0)):
                ref = V.per_image(r64)
                tol = 4.0 * (torch.from_numpy(r32).double() - r64).abs().reshape(B, -1).max(1).values + cond + 2.0 ** -24 * ref.abs()
                assert bool(((got[name].double() - ref).abs() <= tol).all()), name
        ins = {'hr': d['hr'].contiguous()} if prior else dict({k: d[k].contiguous() for k in ('hr', 'xt', 'out', 'scal32')}, rows=rows)
        outs = {'vb': ((B,), torch.float32)} if prior else {'vb': ((B,), torch.float32), 'mse': ((B,), torch.float32)}
        return dict(ins=ins, outs=outs, call=call, check=check, expect=B * 16 * 2 * 8, query=lambda lib: int(lib.sr3_vlb_terms_partials_bytes(B)))
    return Row('prior_bpd' if prior else 'vlb_terms', 'sr3_vlb_terms_partials_bytes', 'sr3_prior_bpd_f32' if prior else 'sr3_vlb_terms_f32', build, align=8)


ROWS = [vlb_terms_row(False), vlb_terms_row(True)]
