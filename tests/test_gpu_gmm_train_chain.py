"""-m gpu: the chain initial_model -> eight EM iterations on the device -> to_gmm() -> conversion -> MLPG on the planted pair of
tests/gmm_train_rule.py (source rows, and target rows that are a planted affine map of the source per mixture plus noise): training
lowers the error against the planted target -- the condition test_gmm_train_rule.py shows the rule meets on the same data -- and
wc_gmm_create takes what model_host returns."""
import numpy as np
import pytest

import features_rule as fr
import gmm_rule as gm
import gmm_train_rule as tr

pytestmark = pytest.mark.gpu

DX = DY = 6
ND, ORDERS = 3, 2          # the target's six columns as MLPG's mgc block: three statics and their three deltas


def test_training_lowers_the_conversion_error_and_its_model_converts(tmp_path):
    import torch
    import world_class_amd as w
    from world_class_amd import features as ft, gmm, gmm_train as gt
    w.lib().wc_set_device(0)
    joint = tr.planted_pair()
    n, D = joint.shape
    assert (n, D) == (2000, DX + DY)
    start = gt.initial_model(joint, 4, 1)
    d_joint = torch.from_numpy(joint.ravel().copy()).cuda()
    W2, W1 = fr.width(ND, 0, ORDERS), fr.width(ND, 0, 1)

    def converted(g):
        """the joint rows' source part through convert into MLPG's rows (every other column: mean 0, variance 1), then MLPG.  The planted
        deltas are columns of their own, not the deltas of the planted statics, so their variances are set to +inf: MLPG drops them and
        generates from the static observations"""
        d_mean = torch.zeros(n * W2, dtype=torch.float64, device="cuda")
        d_var = torch.ones(n * W2, dtype=torch.float64, device="cuda")
        d_static = torch.full((n * W1,), np.nan, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        g.convert(n, d_joint, D, d_mean, d_var, W2)
        w.lib().wc_synchronize()
        converted_var = d_var.cpu().numpy().reshape(n, W2)
        d_var.view(n, W2)[:, ND:2 * ND] = float("inf")
        torch.cuda.synchronize()
        ft.mlpg([n], ND, 0, ORDERS, d_mean, d_var, d_static, var_per_frame=True)
        w.lib().wc_synchronize()
        return d_mean.cpu().numpy().reshape(n, W2), converted_var, d_var.cpu().numpy().reshape(n, W2), d_static.cpu().numpy().reshape(n, W1)

    def errors(model):
        g = gmm.Gmm(*model, DX)          # wc_gmm_create accepts the arrays
        mean, var, var_mlpg, static = converted(g)
        want_mean, want_var, _, _ = gm.convert(gm.prepare(*model, DX, DY), joint[:, :DX])
        assert np.array_equal(mean[:, :DY], want_mean) and np.array_equal(var[:, :DY], want_var)
        assert np.array_equal(static[:, :ND], fr.mlpg([n], ND, 0, ORDERS, mean, var_mlpg, True)[:, :ND]) and np.isfinite(static).all()
        g.close()
        return float(((mean[:, :DY] - joint[:, DX:]) ** 2).mean()), float(((static[:, :ND] - joint[:, DX:DX + ND]) ** 2).mean())

    t = gt.GmmTrainer(4, DX, DY)
    t.set_model(*start)
    infos = t.fit(d_joint, n, D, 8)
    assert [i["n_live"] for i in infos] == [n] * 8 and all(i["n_kept"] == 0 for i in infos)
    ll = [i["loglik"] for i in infos]
    assert all(b >= a for a, b in zip(ll, ll[1:])), ll
    trained = t.model()
    g = t.to_gmm()
    assert (g.n_mix, g.dx, g.dy) == (4, DX, DY)
    own = g.prepared()
    again = gmm.Gmm(*trained, DX)
    assert all(np.array_equal(a, b) for a, b in zip(own, again.prepared()))       # to_gmm is create on model_host's arrays
    g.close()
    again.close()
    before, after = errors(start), errors(trained)
    print("mean squared error of the converted rows / of MLPG's statics: before", before, "after", after)
    assert after[0] < 0.5 * before[0]          # the margin test_gmm_train_rule.py shows for the rule
    assert after[1] < 0.5 * before[1]
    t.close()
