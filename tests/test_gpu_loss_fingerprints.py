"""GPU: one solve per path through the loss kernels and the certificate launches of csrc/zf_kernels_loss.h, csrc/zf_kernels_gap.h
and csrc/zf_loss_dispatch.h, each compared bit for bit with what the PARENT commit's library computed (the pattern of
tests/test_gpu_sweep_fingerprints.py, whose OPTS, _hex and _sha are used here).

The parent had a rows kernel, a pair of launchers and a gap tail per loss; this tree builds them from one body each.  Per id the
fingerprint is zf_solver_ls_plan (6 values), sha256 of the bytes of x_12 (12 iterations from x0 = 0, lr = 1, tol = 0, momentum),
the doubles of zf_solver_duality_gap at that iterate (10 where l2 > 0, else 8), sha256 of jac_f(x_12), f(x_12), and the doubles
of the standalone duality_gap(x_12).  The live and the standalone gap are also asserted byte-equal on every id where they were
at the parent (LIVE_EQUALS_ALONE).

The ids:
  trial-side rows kernel, both shapes    the seven forms (logistic, Huber, Poisson; square, logistic, Huber, Poisson with row
                                         weights) on 2000 x 5000 (one workgroup of 1024 threads, a second trip for threads
                                         0 .. 975; n > 4096: chunked n-passes in the live gap) and on 40000 x 500 (40 chunks and
                                         the finish kernel)
  the l2 > 0 tail                        the four losses on 1000 x 257 (one workgroup over n) and on 2000 x 5000 (chunked n: the
                                         third row of chunk sums), l2 = lam as enet_cases picks it
  weighted KL, wide, elastic net         weighted logistic, l2 = lam, 40000 x 500
  penalty factors                        logistic with positive factors on 1000 x 257: the scaling pass between rows and tail
  dense classes                          the four losses on the dense 1000 x 257 matrix: the same kernels
The real-valued weights are about one fifth zeros, which puts the select of a row that is not there on the path.  Huber ids: the
share of rows clipped at x_12 lies strictly between 0 and 1 (both branches of the clip are summed)."""
import functools
import json

import numpy as np
import pytest

import enet_cases as E
import huber_cases as H
import penalty_cases as PF
import sparse_cases as S
import weight_cases as W
from test_gpu_sweep_fingerprints import OPTS, _hex, _sha

pytestmark = pytest.mark.gpu

CASES = {"small1": S.SMALL[1], "small2": S.SMALL[2], "tall": S.TALL}   # 2000 x 5000, 1000 x 257, 40000 x 500
LOSSES = ("square", "logistic", "huber", "poisson")
FORMS7 = [(loss, False) for loss in LOSSES[1:]] + [(loss, True) for loss in LOSSES]

# id -> (loss, case, storage, row weights, l2 > 0, penalty factors)
TABLE = {}
for _loss, _w in FORMS7:
    for _case in ("small1", "tall"):
        TABLE[f"{'w-' if _w else ''}{_loss}-{_case}"] = (_loss, _case, "csr", _w, False, False)
for _loss in LOSSES:
    for _case in ("small2", "small1"):
        TABLE[f"{_loss}-l2-{_case}"] = (_loss, _case, "csr", False, True, False)
TABLE["w-logistic-l2-tall"] = ("logistic", "tall", "csr", True, True, False)
TABLE["logistic-pf-small2"] = ("logistic", "small2", "csr", False, False, True)
for _loss in LOSSES:
    TABLE[f"{_loss}-dense-small2"] = (_loss, "small2", "dense", False, False, False)
assert len(TABLE) == 28

# Recorded from the library of the parent commit 232cf83 ("Dispatch the two matrix sweeps in one header for solver and
# evaluations") on an MI355X, loaded through ZF_LIB_PATH in a fresh process:
# [ls_plan, sha256(x_12), live gap, sha256(jac_f(x_12)), f(x_12), standalone gap]
PARENT = {
    "logistic-small1": [[5, 32, 16, 1, 1, 0], "26b2ac76f6f9aa186d26a69ed3b9b59c3658a0eef6b91519cc8c4af7f1152a6f",
        ["0x1.49aab5a95feefp+10", "0x1.da9e01cea1377p+9", "0x1.716ed3083d4cap+8", "0x1.a46550d71d989p-2", "0x1.ec4a52c4aae9fp+2", "0x1.2a3197a0fbdf4p+10", "0x1.f791e08640fb0p+6", "0x1.3920db9dca107p+8"],
        "652ed3ac0584621ef21717b35571d46488c5cb2ba0109cc95fba5e3093307ae8", "0x1.2a3197a0fbdf4p+10",
        ["0x1.49aab5a95feefp+10", "0x1.da9e01cea1377p+9", "0x1.716ed3083d4cap+8", "0x1.a46550d71d989p-2", "0x1.ec4a52c4aae9fp+2", "0x1.2a3197a0fbdf4p+10", "0x1.f791e08640fb0p+6", "0x1.3920db9dca107p+8"]],
    "logistic-tall": [[5, 4, 64, 1, 1, 0], "6505dff563ad24712bc0ee681e649f61d988a240ae1a3024e2b295b43137a86b",
        ["0x1.aedcc2f443888p+14", "0x1.0f520eb63df32p+13", "0x1.2733bb99248eep+14", "0x1.d08a9271a73eap-4", "0x1.105bbe84ad82bp+6", "0x1.ae72d36b7d1a9p+14", "0x1.a7be2319b7a59p+4", "0x1.2716423cd7fd0p+14"],
        "5a269e13fc4ab1301d1f652ac8b16df3e11c107249b384c2feef6af531557424", "0x1.ae72d36b7d1a9p+14",
        ["0x1.aedcc2f443888p+14", "0x1.0f520eb63df32p+13", "0x1.2733bb99248eep+14", "0x1.d08a9271a73eap-4", "0x1.105bbe84ad82bp+6", "0x1.ae72d36b7d1a9p+14", "0x1.a7be2319b7a59p+4", "0x1.2716423cd7fd0p+14"]],
    "huber-small1": [[5, 32, 16, 1, 1, 0], "f54e3346d094a19bd95483ea30d6418c3901cc1d5c0469b7a9c4a8bc484dc11a",
        ["0x1.12c312fa56aeep+2", "0x1.cfb66d170fd77p-2", "0x1.eb8f5851cb62cp+1", "0x1.a93e6cf2ded21p-4", "0x1.9ca83a5f5995cp-3", "0x1.10f0565803022p+2", "0x1.d2bca253acbacp-6", "0x1.e8b445f16ead6p+1"],
        "a432fcdeb53e481add328223f2be88ff57148d2bd42e61065d454d407e7b8719", "0x1.10f0565803022p+2",
        ["0x1.12c312fa56aeep+2", "0x1.cfb66d170fd77p-2", "0x1.eb8f5851cb62cp+1", "0x1.a93e6cf2ded21p-4", "0x1.9ca83a5f5995cp-3", "0x1.10f0565803022p+2", "0x1.d2bca253acbacp-6", "0x1.e8b445f16ead6p+1"]],
    "huber-tall": [[5, 4, 64, 1, 1, 0], "ab887eec2468016fbabc72fbafb161e92bc2f49b554d324960494a9f0a6eef9e",
        ["0x1.49d89330b8e18p+5", "0x1.1e5c75144c9dcp+2", "0x1.260d048e2f4dep+5", "0x1.a48497259608ap-4", "0x1.40c840980a6b4p+0", "0x1.3fe00885f4642p+5", "0x1.3f1155588fac8p+0", "0x1.1e4f79cf182c2p+5"],
        "64b412506be346bcc3d37663edbe907cf80222afa0efee488ecf33571ef9758c", "0x1.3fe00885f4642p+5",
        ["0x1.49d89330b8e18p+5", "0x1.1e5c75144c9dcp+2", "0x1.260d048e2f4dep+5", "0x1.a48497259608ap-4", "0x1.40c840980a6b4p+0", "0x1.3fe00885f4642p+5", "0x1.3f1155588fac8p+0", "0x1.1e4f79cf182c2p+5"]],
    "poisson-small1": [[5, 32, 16, 1, 1, 0], "438e1873a52882d130ed260ccd901ad144dc4dad683f8f8a49f3bb2a7b9e326f",
        ["0x1.e23b9ca693d0cp+10", "0x1.a7e9a7ebb8a8bp+10", "0x1.d28fa5d6d9404p+7", "0x1.f81618094f5b8p-2", "0x1.8645a78cad2f7p+3", "0x1.c1abe7840eaa4p+10", "0x1.047da9142933cp+7", "0x1.73dbf38156e1fp+7"],
        "4156afb1e693388821aeb9164e3836422a58ad57d57409a3404ccfaa8906231f", "0x1.c1abe7840eaa4p+10",
        ["0x1.e23b9ca693d0cp+10", "0x1.a7e9a7ebb8a8bp+10", "0x1.d28fa5d6d9404p+7", "0x1.f81618094f5b8p-2", "0x1.8645a78cad2f7p+3", "0x1.c1abe7840eaa4p+10", "0x1.047da9142933cp+7", "0x1.73dbf38156e1fp+7"]],
    "poisson-tall": [[5, 4, 64, 1, 1, 0], "a1b4923b904543b0d14d44173a1880bcd297bf7d584a7e78145132c58181ec3f",
        ["0x1.3812617b6672cp+15", "0x1.80e009e3d0738p+14", "0x1.de897225f8e3fp+13", "0x1.0f2ca101ef640p-3", "0x1.a147e94057992p+6", "0x1.37de8d208d4a4p+15", "0x1.9ea2d6c9443d0p+4", "0x1.de07db1e32d6ep+13"],
        "54a45cfeb192a118aa68e90f88aab06774c0bea51de2e2d7fa570e02a5156207", "0x1.37de8d208d4a4p+15",
        ["0x1.3812617b6672cp+15", "0x1.80e009e3d0738p+14", "0x1.de897225f8e3fp+13", "0x1.0f2ca101ef640p-3", "0x1.a147e94057992p+6", "0x1.37de8d208d4a4p+15", "0x1.9ea2d6c9443d0p+4", "0x1.de07db1e32d6ep+13"]],
    "w-square-small1": [[5, 32, 16, 1, 1, 0], "bd279deab487fa4a9ad95680ec83eab805963f20cc3409672579877f4fb90c2d",
        ["0x1.1dd2997aafbc1p+5", "0x1.ea1e0096c978ap+4", "0x1.461cc97a57fe5p+2", "0x1.6a1e262f3307dp-1", "0x1.88188f425ee60p+2", "0x1.68314a5ae11e7p+3", "0x1.878c8dc7eee8ep+4", "0x1.eddf6cbe11956p-1"],
        "aadbf24e79488c83151c8962ec95bbf0fde3a13036d82ef55ff9a7a6abead113", "0x1.68314a5ae11e7p+3",
        ["0x1.1dd2997aafbc1p+5", "0x1.ea1e0096c978ap+4", "0x1.461cc97a57fe5p+2", "0x1.6a1e262f3307dp-1", "0x1.88188f425ee60p+2", "0x1.68314a5ae11e7p+3", "0x1.878c8dc7eee8ep+4", "0x1.eddf6cbe11956p-1"]],
    "w-square-tall": [[5, 4, 64, 1, 1, 0], "864c585988440e0fc36a4e451e055808ebf5321944718b1f5e9b519872614b56",
        ["0x1.1e5bc1e9603b5p+8", "0x1.1e25d1efd3d41p+8", "0x1.af7fcc633a930p-3", "0x1.ff9079bce1a5bp-1", "0x1.f006a5e3e42fdp+4", "0x1.c66da8f607b72p+5", "0x1.cb1c19953e88dp+7", "0x1.58f93880d30f7p-15"],
        "15657ab9ed5eb0727eabc01e5661d5da9ccd06188686cc03f462259d58c482c3", "0x1.c66da8f607b72p+5",
        ["0x1.1e5bc1e9603b5p+8", "0x1.1e25d1efd3d41p+8", "0x1.af7fcc633a930p-3", "0x1.ff9079bce1a5bp-1", "0x1.f006a5e3e42fdp+4", "0x1.c66da8f607b72p+5", "0x1.cb1c19953e88dp+7", "0x1.58f93880d30f7p-15"]],
    "w-logistic-small1": [[5, 32, 16, 1, 1, 0], "a8d4848a38ee52c93d5f79a104b185df10b0ee1a034e09fa09322d79fcc416d2",
        ["0x1.39dfca42c2db5p+10", "0x1.e4306f1215847p+9", "0x1.1f1e4ae6e0645p+8", "0x1.ed3948b42f895p-2", "0x1.a399a3abfde24p+2", "0x1.022132fe9b6c3p+10", "0x1.bdf4ba213b793p+7", "0x1.9432f610297bdp+7"],
        "b1492e4f53deba08b5b7bd0bb5c83a4233691fd14c180cd717eea2df156c1197", "0x1.022132fe9b6c3p+10",
        ["0x1.39dfca42c2db5p+10", "0x1.e4306f1215847p+9", "0x1.1f1e4ae6e0645p+8", "0x1.ed3948b42f895p-2", "0x1.a399a3abfde24p+2", "0x1.022132fe9b6c3p+10", "0x1.bdf4ba213b793p+7", "0x1.9432f610297bdp+7"]],
    "w-logistic-tall": [[5, 4, 64, 1, 1, 0], "fdb25859f8d37f350366f53f14249e14723b732404a382ddbfdb413157464ab3",
        ["0x1.af8a91da9a042p+14", "0x1.07799c405fc13p+13", "0x1.2bcdc3ba6a238p+14", "0x1.bd5f515df8b7ep-4", "0x1.1c14aceefc135p+6", "0x1.af0607cd2b15ep+14", "0x1.09141adddc8d6p+5", "0x1.2b98f921ebe17p+14"],
        "318398ce325c62be41f1d24364200b9e8190915c2f1f54c599c63781f71efea2", "0x1.af0607cd2b15ep+14",
        ["0x1.af8a91da9a042p+14", "0x1.07799c405fc13p+13", "0x1.2bcdc3ba6a238p+14", "0x1.bd5f515df8b7ep-4", "0x1.1c14aceefc135p+6", "0x1.af0607cd2b15ep+14", "0x1.09141adddc8d6p+5", "0x1.2b98f921ebe17p+14"]],
    "w-huber-small1": [[5, 32, 16, 1, 1, 0], "e1a5bb934c3c0d6661cc58ddf67171dcf8f8541dde96bf38895dca48179463ae",
        ["0x1.0a7d9a4de1a49p+2", "0x1.b24afe18b1494p-2", "0x1.deb1d4d8ad201p+1", "0x1.9a0b0c8163f36p-4", "0x1.abf4696f8568cp-3", "0x1.08307d31ab09bp+2", "0x1.268e8e1b4d6d8p-5", "0x1.db1247c022bb2p+1"],
        "af7accd4390915def74d6c82fa0eb0cc70c2885a300ae507fa909fca938046ff", "0x1.08307d31ab09bp+2",
        ["0x1.0a7d9a4de1a49p+2", "0x1.b24afe18b1494p-2", "0x1.deb1d4d8ad201p+1", "0x1.9a0b0c8163f36p-4", "0x1.abf4696f8568cp-3", "0x1.08307d31ab09bp+2", "0x1.268e8e1b4d6d8p-5", "0x1.db1247c022bb2p+1"]],
    "w-huber-tall": [[5, 4, 64, 1, 1, 0], "b8f2e65d3ab5b528955e71b1b848371a1b38ddcb79f2b138c46d74e6d8b5081e",
        ["0x1.749c571d84deap+5", "0x1.234fb1adc050fp+2", "0x1.503260e7ccd47p+5", "0x1.88abb2aeba93cp-4", "0x1.57880490e4692p+0", "0x1.748c7ac5cc9dep+5", "0x1.fb8af708176f0p-8", "0x1.502c7b9de48bdp+5"],
        "3f8e185e4067bb69cb5f78cc805ee6432f373d96562d8a5b08be4f3f723681f5", "0x1.748c7ac5cc9dep+5",
        ["0x1.749c571d84deap+5", "0x1.234fb1adc050fp+2", "0x1.503260e7ccd47p+5", "0x1.88abb2aeba93cp-4", "0x1.57880490e4692p+0", "0x1.748c7ac5cc9dep+5", "0x1.fb8af708176f0p-8", "0x1.502c7b9de48bdp+5"]],
    "w-poisson-small1": [[5, 32, 16, 1, 1, 0], "65cdcf342652d290758827f2764e8e8a98910f5bd491683dda4c3097f46ba0e1",
        ["0x1.d6791abc84532p+10", "0x1.a0099c8e37cd5p+10", "0x1.b37bf172642ddp+7", "0x1.ff36aa6e15dfdp-2", "0x1.80d4bc13dd561p+3", "0x1.a9263512fb378p+10", "0x1.6a972d4c48dcdp+7", "0x1.2928901104a51p+7"],
        "4fd36c0699302d16156cc78fa85c10df37a8ee854667881dc5dec9171afa5e84", "0x1.a9263512fb378p+10",
        ["0x1.d6791abc84532p+10", "0x1.a0099c8e37cd5p+10", "0x1.b37bf172642ddp+7", "0x1.ff36aa6e15dfdp-2", "0x1.80d4bc13dd561p+3", "0x1.a9263512fb378p+10", "0x1.6a972d4c48dcdp+7", "0x1.2928901104a51p+7"]],
    "w-poisson-tall": [[5, 4, 64, 1, 1, 0], "0b8aeb06eb0f277573c0867076e334d02a42b1a877d091d280ad05194c924457",
        ["0x1.37c9eef5459d1p+15", "0x1.d9ebd48863525p+14", "0x1.2b5012c44fcffp+13", "0x1.2e3e27500c038p-2", "0x1.76632805b1f62p+5", "0x1.36d4afbb2f15ap+15", "0x1.ea7e742d0eecap+6", "0x1.29113dbaf4718p+13"],
        "5f1ca2161c0b3b03cbb4de4e8f8eb56f8a3187419d0fdbc3848c4b264c3dbb70", "0x1.36d4afbb2f15ap+15",
        ["0x1.37c9eef5459d1p+15", "0x1.d9ebd48863525p+14", "0x1.2b5012c44fcffp+13", "0x1.2e3e27500c038p-2", "0x1.76632805b1f62p+5", "0x1.36d4afbb2f15ap+15", "0x1.ea7e742d0eecap+6", "0x1.29113dbaf4718p+13"]],
    "square-l2-small2": [[5, 8, 32, 0, 1, 0], "f01b1a129db1a4ed07b1f6725000e4ce929112a269ea17c97e2dec76d302305d",
        ["0x1.28936653e9f04p+7", "0x1.c7bf519e9b3edp+6", "0x1.12cef61271435p+5", "0x1.12bebe48c7ef3p-1", "0x1.0c4dffdd3eaaap+4", "0x1.8ea69f655b1a8p+5", "0x1.22af312012da5p+6", "0x1.56684e5646eb8p+3", "0x1.9c912f544de3bp+4", "0x1.625c3f096ea5dp+2"],
        "30bf9ba4c3e5dff45673419fef4818a09b585b1471f589f83dcf73584803fc90", "0x1.8ea69f655b1a8p+5",
        ["0x1.28936653e9f04p+7", "0x1.c7bf519e9b3edp+6", "0x1.12cef61271435p+5", "0x1.12bebe48c7ef3p-1", "0x1.0c4dffdd3eaaap+4", "0x1.8ea69f655b1a8p+5", "0x1.22af312012da5p+6", "0x1.56684e5646eb8p+3", "0x1.9c912f544de3bp+4", "0x1.625c3f096ea5dp+2"]],
    "square-l2-small1": [[5, 32, 16, 1, 1, 0], "e313b7d26c33ca2d3bd983965a892cf70b6a413dd5120c6ce92ca516b38da0fc",
        ["0x1.13c4f5547e0a0p+6", "0x1.7dc8f28c5bc41p+4", "0x1.68a57162ce31fp+5", "0x1.6d90f0f2789eep-3", "0x1.8465b3ac0ae70p+4", "0x1.b4da5a5ca2229p+5", "0x1.b024cdda02862p+3", "0x1.26d0f2592cd55p+5", "0x1.a997357653f71p-1", "0x1.1f3737a1f0bc1p-1"],
        "fffeafd0bd855e204b9bbf065cf430f2c41e5e117698eda5822bd185572cfe3b", "0x1.b4da5a5ca2229p+5",
        ["0x1.13c4f5547e0a0p+6", "0x1.7dc8f28c5bc41p+4", "0x1.68a57162ce31fp+5", "0x1.6d90f0f2789eep-3", "0x1.8465b3ac0ae70p+4", "0x1.b4da5a5ca2229p+5", "0x1.b024cdda02862p+3", "0x1.26d0f2592cd55p+5", "0x1.a997357653f71p-1", "0x1.1f3737a1f0bc1p-1"]],
    "logistic-l2-small2": [[5, 8, 32, 0, 1, 0], "4d3d693b316b14662bf0bfa45525f8a82d095594ef2b7196f43f4542062ebef2",
        ["0x1.207b071f348fap+9", "0x1.b89d272ecbcaap+8", "0x1.10b1ce1f3aa95p+7", "0x1.d2f04676bdd4fp-2", "0x1.a83e87bf28de9p+2", "0x1.ec6d27d8e7058p+8", "0x1.0998e66f4aee9p+6", "0x1.af10ed83429a8p+6", "0x1.222acc9af5e1ep+4", "0x1.577d87d106c8bp+2"],
        "c12394cccbcce9bf751a8d1c303dc95147f49184cf6b6344eaa60ed41bdb534f", "0x1.ec6d27d8e7058p+8",
        ["0x1.207b071f348fap+9", "0x1.b89d272ecbcaap+8", "0x1.10b1ce1f3aa95p+7", "0x1.d2f04676bdd4fp-2", "0x1.a83e87bf28de9p+2", "0x1.ec6d27d8e7058p+8", "0x1.0998e66f4aee9p+6", "0x1.af10ed83429a8p+6", "0x1.222acc9af5e1ep+4", "0x1.577d87d106c8bp+2"]],
    "logistic-l2-small1": [[5, 32, 16, 1, 1, 0], "9adb42a34882c14ae3f476b06169db75c78317cd71c9119b086ef1301c727239",
        ["0x1.4bf3c0362265fp+10", "0x1.feecca49bab11p+9", "0x1.31f56c4514356p+8", "0x1.dc5f6cb286c25p-2", "0x1.b27162f95f645p+2", "0x1.2d6e6798c8e2cp+10", "0x1.d1abd6d296c36p+6", "0x1.00f7aee61dcb8p+8", "0x1.6a9b30301705ep+2", "0x1.9ed3517f23f66p+0"],
        "6b225c85026dc8c9c615c43b410f0fff4f42a1f91cb3a66bd0fd9a7cef5606c9", "0x1.2d6e6798c8e2cp+10",
        ["0x1.4bf3c0362265fp+10", "0x1.feecca49bab11p+9", "0x1.31f56c4514356p+8", "0x1.dc5f6cb286c25p-2", "0x1.b27162f95f645p+2", "0x1.2d6e6798c8e2cp+10", "0x1.d1abd6d296c36p+6", "0x1.00f7aee61dcb8p+8", "0x1.6a9b30301705ep+2", "0x1.9ed3517f23f66p+0"]],
    "huber-l2-small2": [[5, 8, 32, 0, 1, 0], "7f26f64b015c8afda5df91dc0ac941010f9db709a2ca380770f2805ebf1f60d5",
        ["0x1.13e304cec82bap+7", "0x1.913781074cb80p+4", "0x1.c378295bbd291p+6", "0x1.1b90472fad5dfp-3", "0x1.018aba5f005e0p+3", "0x1.ee58dc6d673b7p+6", "0x1.6b2b0fa8a9a17p+3", "0x1.a4cfc86ab2787p+6", "0x1.80f967627cf23p+1", "0x1.1dbf96146da1cp+1"],
        "05f6946689c3d6831eadc64a615b338ce6da0ce8f2c656033b773683dc536a49", "0x1.ee58dc6d673b7p+6",
        ["0x1.13e304cec82bap+7", "0x1.913781074cb80p+4", "0x1.c378295bbd291p+6", "0x1.1b90472fad5dfp-3", "0x1.018aba5f005e0p+3", "0x1.ee58dc6d673b7p+6", "0x1.6b2b0fa8a9a17p+3", "0x1.a4cfc86ab2787p+6", "0x1.80f967627cf23p+1", "0x1.1dbf96146da1cp+1"]],
    "huber-l2-small1": [[5, 32, 16, 1, 1, 0], "41b8a232e427cfe1f4bb74d0dc93fe4b2140d44615488171dd78edc2d77c0baa",
        ["0x1.12c37aaa5b814p+2", "0x1.cff58ab2e71eep-2", "0x1.eb8843fe5a1ecp+1", "0x1.a978115e6da63p-4", "0x1.9c70524d89e68p-3", "0x1.10f0aefff4ea8p+2", "0x1.d29316be900c1p-6", "0x1.e8ad2417a86c2p+1", "0x1.c49d403543bf4p-17", "0x1.6b77cbdbafa49p-17"],
        "5d1dd996075d489df323379790c42382ef8083bfd5308bc46891cd1b96950ff5", "0x1.10f0aefff4ea8p+2",
        ["0x1.12c37aaa5b814p+2", "0x1.cff58ab2e71eep-2", "0x1.eb8843fe5a1ecp+1", "0x1.a978115e6da63p-4", "0x1.9c70524d89e68p-3", "0x1.10f0aefff4ea8p+2", "0x1.d29316be900c1p-6", "0x1.e8ad2417a86c2p+1", "0x1.c49d403543bf4p-17", "0x1.6b77cbdbafa49p-17"]],
    "poisson-l2-small2": [[5, 8, 32, 0, 1, 0], "d20c7a1df91003f2727835c06adbd9e05323e52d03e889e73657dffcafe2c25e",
        ["0x1.cda23e04099dap+9", "0x1.8c3f2c0da99d2p+9", "0x1.058c47d980014p+7", "0x1.f23c217b75fccp-2", "0x1.fc197f9991b2cp+2", "0x1.b41b87d6eb641p+9", "0x1.7a06325428bc8p+5", "0x1.bd96246f7df87p+6", "0x1.e65307dbadbeap+1", "0x1.0069aa1a6bac8p+0"],
        "b19bad8a825afc62c03cd9ce99cd2ca3cfb62d98124c50d983fa41e365c71fb2", "0x1.b41b87d6eb641p+9",
        ["0x1.cda23e04099dap+9", "0x1.8c3f2c0da99d2p+9", "0x1.058c47d980014p+7", "0x1.f23c217b75fccp-2", "0x1.fc197f9991b2cp+2", "0x1.b41b87d6eb641p+9", "0x1.7a06325428bc8p+5", "0x1.bd96246f7df87p+6", "0x1.e65307dbadbeap+1", "0x1.0069aa1a6bac8p+0"]],
    "poisson-l2-small1": [[5, 32, 16, 1, 1, 0], "b2b2f2f3fac2c0dec8c689f2de250eafca2ee1cf872a96165278edf455a66e87",
        ["0x1.e35c241451c98p+10", "0x1.adf2f112b1ac8p+10", "0x1.ab49980d00e82p+7", "0x1.08917d4d5b301p-1", "0x1.73cbbdee30380p+3", "0x1.c33030c471ec3p+10", "0x1.f67e188781c7bp+6", "0x1.528a71d7d54bfp+7", "0x1.88238ecf8191fp+1", "0x1.6e541307b7f7ep-1"],
        "81ab866987b2fbe0979cfd28a6df304f5c9268a916fade2b2b656ff95227940e", "0x1.c33030c471ec3p+10",
        ["0x1.e35c241451c98p+10", "0x1.adf2f112b1ac8p+10", "0x1.ab49980d00e82p+7", "0x1.08917d4d5b301p-1", "0x1.73cbbdee30380p+3", "0x1.c33030c471ec3p+10", "0x1.f67e188781c7bp+6", "0x1.528a71d7d54bfp+7", "0x1.88238ecf8191fp+1", "0x1.6e541307b7f7ep-1"]],
    "w-logistic-l2-tall": [[5, 4, 64, 1, 1, 0], "b165dc6ef9205823b858fd861258df1d7379e79e7fcbfdd07c1a4b7a0908e2e7",
        ["0x1.af9719d570fcap+14", "0x1.0af2ec2321cd2p+13", "0x1.2a1da3c3e0163p+14", "0x1.c55b95629c232p-4", "0x1.1713b53e2d10dp+6", "0x1.af0db6029ba1cp+14", "0x1.064ee50f421f0p+5", "0x1.29e495c727c4ep+14", "0x1.8f18136e72df9p+0", "0x1.3ba329ab82340p+0"],
        "cb9f7b1db9cbb8a64db7709701ec5ebf7377d3e047d6feeac0cfd9ed2a553954", "0x1.af0db6029ba1cp+14",
        ["0x1.af9719d570fcap+14", "0x1.0af2ec2321cd2p+13", "0x1.2a1da3c3e0163p+14", "0x1.c55b95629c232p-4", "0x1.1713b53e2d10dp+6", "0x1.af0db6029ba1cp+14", "0x1.064ee50f421f0p+5", "0x1.29e495c727c4ep+14", "0x1.8f18136e72df9p+0", "0x1.3ba329ab82340p+0"]],
    "logistic-pf-small2": [[5, 8, 32, 0, 1, 0], "ac71c1fccc0d4ae89dfb78cadf719db7e1676883870686fe2d7d8e7544b84015",
        ["0x1.2f348d011aa94p+9", "0x1.287256fafb104p+8", "0x1.35f6c3073a423p+8", "0x1.cab942c13738ap-3", "0x1.afd77963ff6dfp+3", "0x1.0a561514d7706p+9", "0x1.26f3bf6219c6fp+6", "0x1.03e5c1390c3bcp+8"],
        "f52d9cc45f8dde6bd7a8eb13da0a2345f2746bb19b93937dc375ac41c663c5e7", "0x1.0a561514d7706p+9",
        ["0x1.2f348d011aa94p+9", "0x1.287256fafb104p+8", "0x1.35f6c3073a423p+8", "0x1.cab942c13738ap-3", "0x1.afd77963ff6dfp+3", "0x1.0a561514d7706p+9", "0x1.26f3bf6219c6fp+6", "0x1.03e5c1390c3bcp+8"]],
    "square-dense-small2": [[4, 3, 63, 16, 1, 0], "2c37994a31f71df6ec33838da6d24431c14ce8b79db52ffbcb19173af5881789",
        ["0x1.cb50758e50d98p+6", "0x1.40b1ba4edd01fp+6", "0x1.153d767ee7af2p+5", "0x1.bc2fbdc5d6176p-2", "0x1.4be9739242422p+4", "0x1.0fa704e86c587p+5", "0x1.437cf31a1aad5p+6", "0x1.5c60af477b944p+3"],
        "341f7813cacb7764b1ea1335dfc672d180f0af20fc3f2a9131187fe138c3cf88", "0x1.0fa704e86c587p+5",
        ["0x1.cb50758e50d98p+6", "0x1.40b1ba4edd01fp+6", "0x1.153d767ee7af2p+5", "0x1.bc2fbdc5d6176p-2", "0x1.4be9739242422p+4", "0x1.0fa704e86c587p+5", "0x1.437cf31a1aad5p+6", "0x1.5c60af477b944p+3"]],
    "logistic-dense-small2": [[4, 3, 63, 16, 1, 0], "e316d1847d15c36cad1136c18f4cdbf5917b73a544aa605f062a09b996acf0ba",
        ["0x1.130636c6b06adp+9", "0x1.6a7a3191a5710p+8", "0x1.772477f776c95p+7", "0x1.5e1932ef3547fp-2", "0x1.1aea2bf3b0688p+3", "0x1.da1ba6495c2aep+8", "0x1.2fc31d1012ab2p+6", "0x1.3ac6a9ed62f21p+7"],
        "4681bb265484e937e74072685d37d35d63f4a56729f6f595d17932c0a2b0b44c", "0x1.da1ba6495c2aep+8",
        ["0x1.130636c6b06adp+9", "0x1.6a7a3191a5710p+8", "0x1.772477f776c95p+7", "0x1.5e1932ef3547fp-2", "0x1.1aea2bf3b0688p+3", "0x1.da1ba6495c2aep+8", "0x1.2fc31d1012ab2p+6", "0x1.3ac6a9ed62f21p+7"]],
    "huber-dense-small2": [[4, 3, 63, 16, 1, 0], "733fc670ec48c8f9174a4a686e16c81eeb192a4892eddb7f353b631c3526d7c9",
        ["0x1.08b2eb86a2094p+7", "0x1.8632e4444b3f7p+4", "0x1.afd91dfc3142bp+6", "0x1.1b5ea8f0540f5p-3", "0x1.01b7d2dde3984p+3", "0x1.e1953c88a3c47p+6", "0x1.7e84d4250270ep+3", "0x1.9a31377f8412ep+6"],
        "0386c35be23cb90d0f9a88f218072714b8f4a492ccee8c12037be7c6cf51baff", "0x1.e1953c88a3c47p+6",
        ["0x1.08b2eb86a2094p+7", "0x1.8632e4444b3f7p+4", "0x1.afd91dfc3142bp+6", "0x1.1b5ea8f0540f5p-3", "0x1.01b7d2dde3984p+3", "0x1.e1953c88a3c47p+6", "0x1.7e84d4250270ep+3", "0x1.9a31377f8412ep+6"]],
    "poisson-dense-small2": [[4, 3, 63, 16, 1, 0], "8ce081c249ee08850f27c42b7434d62126f0d33fa11e851e9bf02be0b61cde4a",
        ["0x1.cb5707f2218eep+9", "0x1.80bac08aa9d4fp+9", "0x1.2a711d9ddee89p+7", "0x1.c9fa2ae4c928bp-2", "0x1.1461b03dd07dfp+3", "0x1.b2c0676b39894p+9", "0x1.896a086e805a7p+5", "0x1.01b025a87b575p+7"],
        "b1eb2a982217078fdb8a89d2669cf1776b9d76fdeb11ad71ac015e008ad3490e", "0x1.b2c0676b39894p+9",
        ["0x1.cb5707f2218eep+9", "0x1.80bac08aa9d4fp+9", "0x1.2a711d9ddee89p+7", "0x1.c9fa2ae4c928bp-2", "0x1.1461b03dd07dfp+3", "0x1.b2c0676b39894p+9", "0x1.896a086e805a7p+5", "0x1.01b025a87b575p+7"]],
}
# ids whose live and standalone gap were byte-equal at the parent
LIVE_EQUALS_ALONE = set(TABLE)


@functools.lru_cache(maxsize=None)
def _data(loss, case):
    """(A csr, b, lam, delta) of a loss on a case - read-only, shared."""
    return PF.make_problem(CASES[case], loss)


def _problem(name):
    from zfista_amd import problems as Z

    loss, case, storage, weighted, enet, factors = TABLE[name]
    A, b, lam, delta = _data(loss, case)
    m, n, _, seed = CASES[case]
    M = W.matrix(A, storage)
    cls = {"square": (Z.SparseLeastSquaresL1, Z.LeastSquaresL1), "logistic": (Z.SparseLogisticL1, Z.LogisticL1),
           "huber": (Z.SparseHuberL1, Z.HuberL1), "poisson": (Z.SparsePoissonL1, Z.PoissonL1)}[loss][storage == "dense"]
    prob = cls(M, b, lam, delta) if loss == "huber" else cls(M, b, lam)
    if weighted:
        prob = prob.with_sample_weight(W.make_weights(m, seed, "real"))
    if enet:
        prob = prob.with_penalty(lam, E.L2_FACTORS[0] * lam)
    if factors:   # (positive: the certificate refuses an unpenalised column)
        prob = prob.with_penalty_factor(PF.make_factors(n, seed, "positive"))
    return prob


def fingerprint(name):
    """[ls_plan (6), sha256(x_12), live gap, sha256(jac_f(x_12)), f(x_12), standalone gap]"""
    import ctypes as C

    from zfista_amd import _lib
    from zfista_amd.problems import DualityGap
    from zfista_amd.proximal_gradient import NativeRun

    prob = _problem(name)
    count = 10 if TABLE[name][4] else 8
    run = NativeRun(prob, np.zeros(prob.n_features), OPTS)
    plan = np.zeros(6, dtype=np.int64)
    _lib.check(run.solver.lib.zf_solver_ls_plan(run.solver.handle, C.c_void_p(_lib.ptr(plan)), plan.size))
    while run.status == _lib.ZF_RUNNING:
        run.advance(4)
    assert run.status == _lib.ZF_MAXITER and run.nit_seen == 12
    x = run.solver.get_x()
    live = np.asarray(run.solver.duality_gap(), dtype=np.float64)
    run.solver.close()
    assert live.size == count
    alone = prob.duality_gap(x)
    alone = [getattr(alone, k) for k in DualityGap.__slots__[:count]]
    return [[int(v) for v in plan], _sha(x), _hex(live[:8]) + _hex(live[8:]), _sha(prob.jac_f(x)), float(prob.f(x)).hex(),
            _hex(alone[:8]) + _hex(alone[8:])], x


@pytest.mark.parametrize("name", list(TABLE))
def test_a_solve_on_each_path_of_the_loss_kernels_computes_the_parent_librarys_bits(name):
    """Plan, x_12, the live certificate, jac_f(x_12), f(x_12) and the standalone certificate of the id equal what the parent
    commit's library gave; the live certificate is the standalone one byte for byte where it was; a Huber id sums rows on
    both sides of delta."""
    got, x = fingerprint(name)
    print(name, json.dumps(got))
    loss, case = TABLE[name][:2]
    if loss == "huber":
        A, b, _, delta = _data(loss, case)
        share = H.clipped_share(A, b, x, delta)
        print(f"{name}: clipped share at x_12 = {share:.4f}")
        assert 0.0 < share < 1.0
    if name in LIVE_EQUALS_ALONE:
        assert got[2] == got[5], "the live gap is the standalone gap, byte for byte"
    assert got == PARENT[name]
