"""GPU: one solve per branch of the two sweep launchers of csrc/zf_matview.h (zf_launch_apply: z = A x; zf_launch_adjoint:
g = factor A^T r), each compared bit for bit with what the PARENT commit's library computed.

The two launchers serve the solver's loop and the evaluations outside it, over five storage forms of A.  Per id the fingerprint is
zf_solver_ls_plan (6 values), sha256 of the bytes of x_12 (12 iterations from x0 = 0, lr = 1, tol = 0, momentum), the 8 doubles of
zf_solver_duality_gap at that iterate, sha256 of jac_f(x_12), and the 8 doubles of the standalone duality_gap(x_12).  The live and
the standalone gap are also asserted byte-equal wherever both take the same column sweep - at the parent that was every id below
(LIVE_EQUALS_ALONE: the MFMA ids too, since both sides take the MFMA sweep for n % 32 == 0).

The sharded branches (the unguarded combine of row blocks, A x into the exchanged vector of column blocks) need several ranks:
tests/test_gpu_sharded_ls.py runs both layouts."""
import functools
import hashlib
import json

import numpy as np
import pytest

import multiresponse_cases as M
import sparse_cases as S

pytestmark = pytest.mark.gpu

OPTS = dict(lr=1.0, tol=0.0, tol_internal=1e-12, max_iter=12, max_iter_internal=100000, max_backtrack_iter=100, warm_start=False,
            decay_rate=0.5, nesterov=True, nesterov_ratio=(0, 0.25), return_all=False, verbose=False, deprecated=False)
GENERAL = {"ZF_LS_SMALL": "0"}   # 96 x 128 would take the fused small-matrix kernels, which are no sweep of the launchers

# id -> (kind, (m, n) of the matrix or the sparse_cases tuple, K, seed, environment)
TABLE = {
    "ls-even": ("ls", (96, 130), 1, 11, {}),           # V = 2, the general path (n % 32 != 0), 12 slices
    "ls-odd": ("ls", (96, 129), 1, 12, {}),            # V = 1
    "ls-one-slice": ("ls", (7, 130), 1, 13, {}),
    "ls-n1": ("ls", (40, 1), 1, 14, {}),               # one column: the partial sweep always runs (there was a guard n / V > 0)
    "ls-mfma": ("ls", (96, 128), 1, 15, GENERAL),
    "ls-valu32": ("ls", (96, 128), 1, 15, dict(GENERAL, ZF_GEMV_MFMA="0")),
    "logistic-mfma": ("logistic", (96, 128), 1, 16, {}),
    "logistic-odd": ("logistic", (96, 129), 1, 17, {}),   # another gfac
    "f32-v4": ("f32", (96, 132), 1, 18, {}),
    "f32-v2": ("f32", (96, 130), 1, 19, {}),
    "f32-v1": ("f32", (96, 129), 1, 20, {}),
    "f32-regrow": ("f32", (512, 20000), 1, 21, {}),    # the fp32 rule takes more slices than zf_solver_create planned: the slab is regrown
    "mr-even": ("mr", (96, 130), 3, 22, {}),
    "mr-odd": ("mr", (96, 129), 3, 23, {}),
    "mr-regrow": ("mr", (512, 10000), 2, 24, {}),      # create plans on 1024 x 20000, the K rule on the matrix itself
    "csr": ("csr", S.SMALL[0], 1, 0, {}),              # no split row
    "csr-split": ("csr", S.SMALL[3], 1, 0, {}),        # 64 x 4099: the smallest shape of sparse_cases with split rows (a row of 4099 > 4096)
    "csr-k3": ("csr", S.SMALL[3], 3, 25, {}),          # the same matrix, 3 responses
    "csr-rem": ("csr-rem", S.TALL, 1, 0, {}),          # acceptance="remainder", 40000 > 2^15 rows: the wide residual with the remainder
}
# slices as zf_solver_create planned them (the fp64 rule on the flattened shape) -> as the setter's rule left them
REGROW = {"f32-regrow": (52, 64), "mr-regrow": (52, 64)}

# Recorded from the library of the parent commit b4cc9f4 ("Resume small-matrix solves bit for bit; test lifecycle on every path")
# on an MI355X, loaded through ZF_LIB_PATH in a fresh process: [ls_plan, sha256(x_12), live gap, sha256(jac_f(x_12)), standalone gap]
PARENT = {
    "ls-even": [[3, 2, 12, 8, 1, 0], "2746b61ed19e897054f7b3bb101fdad322e9e314dcfea530cd754eabdea2fd36",
        ["0x1.4d9ad56dc44a8p+6", "0x1.13637450d4fdap+6", "0x1.d1bb08e77a669p+3", "0x1.cdb6b6ace089fp-1", "0x1.eb118cb851d26p+3", "0x1.2b31c5a2418acp+3", "0x1.28349cb97c192p+6", "0x1.716bf882b335fp-4"],
        "254d7750810cb02640d52b5ed066ae9ba36b07817eec8e0debd3b02140643408",
        ["0x1.4d9ad56dc44a8p+6", "0x1.13637450d4fdap+6", "0x1.d1bb08e77a669p+3", "0x1.cdb6b6ace089fp-1", "0x1.eb118cb851d26p+3", "0x1.2b31c5a2418acp+3", "0x1.28349cb97c192p+6", "0x1.716bf882b335fp-4"]],
    "ls-odd": [[4, 3, 12, 8, 1, 0], "0d3b91b384adac8f7b031189f3eb03cf6b7feeda52d1a4df70c5bdc5a1b59dd8",
        ["0x1.d3f7ed085e050p+6", "0x1.b6793273347e6p+6", "0x1.d7eba952986b5p+2", "0x1.e0982155e4244p-1", "0x1.230ae8b9e447ep+4", "0x1.cce548f45edacp+3", "0x1.9a5b43e9d229ap+6", "0x1.bbefb744a9c77p-5"],
        "a31589ba83273e4386696e15db05793fd1b0c54de55d7f478accb7ee1523586b",
        ["0x1.d3f7ed085e050p+6", "0x1.b6793273347e6p+6", "0x1.d7eba952986b5p+2", "0x1.e0982155e4244p-1", "0x1.230ae8b9e447ep+4", "0x1.cce548f45edacp+3", "0x1.9a5b43e9d229ap+6", "0x1.bbefb744a9c77p-5"]],
    "ls-one-slice": [[3, 2, 1, 7, 1, 0], "12feebd9032bd9b3e0722e8032c735b68ba6dff48acd98ebcc42fb4d0ed6c19f",
        ["0x1.adad2e0111bf4p+2", "0x1.492d64749808ap+2", "0x1.91ff2631e6daap+0", "0x1.50aac3fa195bfp-1", "0x1.0447347456dbbp+2", "0x1.fe1a55113db65p-1", "0x1.6de9e35eea087p+2", "0x1.de8eef661c46bp-4"],
        "f14b7b6b41f2c0b96ef48f0421148a86dbc2a34c1784179fd78e5f8da72e8448",
        ["0x1.adad2e0111bf4p+2", "0x1.492d64749808ap+2", "0x1.91ff2631e6daap+0", "0x1.50aac3fa195bfp-1", "0x1.0447347456dbbp+2", "0x1.fe1a55113db65p-1", "0x1.6de9e35eea087p+2", "0x1.de8eef661c46bp-4"]],
    "ls-n1": [[4, 3, 5, 8, 1, 0], "ed8d87ddb7a97defde3cbc6145d786f2bf3ce87432fe347a68a86d2f2f32fd31",
        ["0x1.cd576c27aecafp-2", "0x1.cd576c27ab82fp-2", "0x1.a40542f961efap-41", "0x1.ffff48a79efd3p-1", "0x1.934964ed61585p+0", "0x1.996af6726c926p-6", "0x1.b3c0bcc08801dp-2", "0x1.a401abed67075p-41"],
        "4b8720fb1bac19f5916f08666a934d3326fd7ba7e0a9970a4ba519e86818cb2d",
        ["0x1.cd576c27aecafp-2", "0x1.cd576c27ab82fp-2", "0x1.a40542f961efap-41", "0x1.ffff48a79efd3p-1", "0x1.934964ed61585p+0", "0x1.996af6726c926p-6", "0x1.b3c0bcc08801dp-2", "0x1.a401abed67075p-41"]],
    "ls-mfma": [[2, 2, 12, 8, 1, 0], "81b57e0dd1fa10c6d44bd59c37eb6efa20c822088a887578b8f6b90047c1dcf0",
        ["0x1.1b7d1f23a3095p+7", "0x1.140f43b9f3b80p+7", "0x1.db76da6bd452bp+1", "0x1.fb63ef35f8827p-1", "0x1.35c2dd013cc1fp+4", "0x1.0a55521356affp+4", "0x1.f464e9c27066ap+6", "0x1.61b3c670e6506p-10"],
        "3d35d32d1347325e2420ec0848a32122ba52a232f799ddf6ee0fe674e29363ec",
        ["0x1.1b7d1f23a3095p+7", "0x1.140f43b9f3b80p+7", "0x1.db76da6bd452bp+1", "0x1.fb63ef35f8827p-1", "0x1.35c2dd013cc1fp+4", "0x1.0a55521356affp+4", "0x1.f464e9c27066ap+6", "0x1.61b3c670e6506p-10"]],
    "ls-valu32": [[3, 2, 12, 8, 1, 0], "81b57e0dd1fa10c6d44bd59c37eb6efa20c822088a887578b8f6b90047c1dcf0",
        ["0x1.1b7d1f23a3095p+7", "0x1.140f43b9f3b80p+7", "0x1.db76da6bd452bp+1", "0x1.fb63ef35f8827p-1", "0x1.35c2dd013cc1fp+4", "0x1.0a55521356affp+4", "0x1.f464e9c27066ap+6", "0x1.61b3c670e6506p-10"],
        "3d35d32d1347325e2420ec0848a32122ba52a232f799ddf6ee0fe674e29363ec",
        ["0x1.1b7d1f23a3095p+7", "0x1.140f43b9f3b80p+7", "0x1.db76da6bd452bp+1", "0x1.fb63ef35f8827p-1", "0x1.35c2dd013cc1fp+4", "0x1.0a55521356affp+4", "0x1.f464e9c27066ap+6", "0x1.61b3c670e6506p-10"]],
    "logistic-mfma": [[2, 2, 12, 8, 1, 0], "1eaf37d42b93a42f8a1648218ad7f2e8270f3078b6fcd3c6bbf4f16033378b66",
        ["0x1.e4f8d33fcb423p+4", "0x1.c20fc1c87aae7p+4", "0x1.17488bba849e0p+1", "0x1.a2557488afbd8p-1", "0x1.3aeea6fa6d6e5p+1", "0x1.b27f74488c752p+3", "0x1.0bb9191b8507ap+4", "0x1.159aee7eae357p-2"],
        "beac42845a8836659d852cc93f3e2bb43168295c9171a38d25f5037b811ab4b2",
        ["0x1.e4f8d33fcb423p+4", "0x1.c20fc1c87aae7p+4", "0x1.17488bba849e0p+1", "0x1.a2557488afbd8p-1", "0x1.3aeea6fa6d6e5p+1", "0x1.b27f74488c752p+3", "0x1.0bb9191b8507ap+4", "0x1.159aee7eae357p-2"]],
    "logistic-odd": [[4, 3, 12, 8, 1, 0], "910b79721dbfc31102a741ed31c1a25d101f9e228e4ea5731bef80ff70ccda6b",
        ["0x1.13a20479c4056p+5", "0x1.f667ce22d7625p+4", "0x1.86e1d68585439p+1", "0x1.93c2c795014c3p-1", "0x1.bd715379d9b26p+1", "0x1.01bf5220eed9cp+4", "0x1.2584b6d299311p+4", "0x1.bc9f218c009f8p-2"],
        "d8bfeb1190a28a1b582642f8039a54b8ab50417d64866b7b8598c19d01c0e039",
        ["0x1.13a20479c4056p+5", "0x1.f667ce22d7625p+4", "0x1.86e1d68585439p+1", "0x1.93c2c795014c3p-1", "0x1.bd715379d9b26p+1", "0x1.01bf5220eed9cp+4", "0x1.2584b6d299311p+4", "0x1.bc9f218c009f8p-2"]],
    "f32-v4": [[6, 4, 12, 8, 1, 0], "a130a433f864b98ee45185913d47a527001df3d209017d4485dd60305f3ff2e2",
        ["0x1.6251f423aacf6p+7", "0x1.3b3b4b5f6235bp+7", "0x1.38b5462244cd8p+4", "0x1.ff7c2ed44691ep-1", "0x1.a1f25d0dd5ccap+4", "0x1.85a4ac8863cdbp+4", "0x1.319d5e929e55bp+7", "0x1.9d3a9112479acp-16"],
        "3b940be9f27c27d8c55f463b188d7988bc9a3cf9406dba965bb008999da53265",
        ["0x1.6251f423aacf6p+7", "0x1.3b3b4b5f6235bp+7", "0x1.38b5462244cd8p+4", "0x1.ff7c2ed44691ep-1", "0x1.a1f25d0dd5ccap+4", "0x1.85a4ac8863cdbp+4", "0x1.319d5e929e55bp+7", "0x1.9d3a9112479acp-16"]],
    "f32-v2": [[7, 5, 12, 8, 1, 0], "57704809801261ab48fe36367a5f94cb14e9082b60e3d243c97f91cd0261b434",
        ["0x1.4f1809f995e13p+6", "0x1.1ea89e8361aa9p+6", "0x1.837b5bb1a1b5dp+3", "0x1.de44d1e5b3344p-1", "0x1.db933c309fbacp+3", "0x1.1c45172dedb00p+3", "0x1.2b8f6713d82b3p+6", "0x1.3bdbffaf82e32p-5"],
        "f6e1a0d64334f0036cfeb76dc457f87ff2d8ce1aafaddc28f0a188e6f1b3b15d",
        ["0x1.4f1809f995e13p+6", "0x1.1ea89e8361aa9p+6", "0x1.837b5bb1a1b5dp+3", "0x1.de44d1e5b3344p-1", "0x1.db933c309fbacp+3", "0x1.1c45172dedb00p+3", "0x1.2b8f6713d82b3p+6", "0x1.3bdbffaf82e32p-5"]],
    "f32-v1": [[8, 6, 12, 8, 1, 0], "3fb952e954566ddee6c751668ccb4edc767c82550fab31c4652bf413c2b6a65f",
        ["0x1.4d68bd16b36c5p+5", "0x1.42c0df3e5266ap+5", "0x1.54fbbb0c20b66p+0", "0x1.e9cfaf2537909p-1", "0x1.83f5e2d97c520p+3", "0x1.985a7800aa75ep+2", "0x1.1a5d6e169e1d9p+5", "0x1.88ac55e58c1ffp-7"],
        "d9e432a934484b2ab950dfc72ce33149a0b4277b563dc147df100186e48e0dde",
        ["0x1.4d68bd16b36c5p+5", "0x1.42c0df3e5266ap+5", "0x1.54fbbb0c20b66p+0", "0x1.e9cfaf2537909p-1", "0x1.83f5e2d97c520p+3", "0x1.985a7800aa75ep+2", "0x1.1a5d6e169e1d9p+5", "0x1.88ac55e58c1ffp-7"]],
    "f32-regrow": [[6, 4, 64, 8, 1, 0], "0e91604fe113bb9aa137026ac6ac89f5fd6f262b1ea507a7c81ccaa0292fe9b4",
        ["0x1.5f2b67dbac2a9p+10", "0x1.15aff7f899d71p+9", "0x1.a8a6d7bebe7e1p+9", "0x1.0668bace12c62p-2", "0x1.47ea4d3edbec4p+8", "0x1.d9c6be78d4345p+8", "0x1.d173707aee3b0p+9", "0x1.0611dd5d2bc82p+8"],
        "5532cc18bd89c32a4f376cc0eab93477deae2485f7caf570dfa7fe7db9119a77",
        ["0x1.5f2b67dbac2a9p+10", "0x1.15aff7f899d71p+9", "0x1.a8a6d7bebe7e1p+9", "0x1.0668bace12c62p-2", "0x1.47ea4d3edbec4p+8", "0x1.d9c6be78d4345p+8", "0x1.d173707aee3b0p+9", "0x1.0611dd5d2bc82p+8"]],
    "mr-even": [[9, 7, 12, 8, 3, 16], "dbd19e74779cbce38743ffb315d64b8946a5a17e8e622c3a0e978f95eaf17408",
        ["0x1.11e643b52131cp+9", "0x1.f83fe95ef8bfdp+8", "0x1.5c64f05a4d1cep+5", "0x1.dc0e066b8228ap-1", "0x1.d7a6f818fdd6ap+4", "0x1.dd69652b0dd5ep+6", "0x1.ac722e1f7eee1p+8", "0x1.2d317a3f53542p-1"],
        "cd362093c9295777e73a0a1515d352e5b5b93093d93ef6a0e9a749915effbc11",
        ["0x1.11e643b52131cp+9", "0x1.f83fe95ef8bfdp+8", "0x1.5c64f05a4d1cep+5", "0x1.dc0e066b8228ap-1", "0x1.d7a6f818fdd6ap+4", "0x1.dd69652b0dd5ep+6", "0x1.ac722e1f7eee1p+8", "0x1.2d317a3f53542p-1"]],
    "mr-odd": [[10, 8, 12, 8, 3, 16], "5098e37b96cfbda87c4c201f99d79031f531955d6124161988245c30a1089447",
        ["0x1.e1dcebbf8bdbcp+9", "0x1.c676ac7be2788p+9", "0x1.b663f43a9632ap+5", "0x1.de4d2cf8f734dp-1", "0x1.54fec792761cbp+5", "0x1.84b5e84bd0ae7p+7", "0x1.80af71ac97b02p+9", "0x1.af1211290d29ap-1"],
        "dd8092eb724d3d29a59ed6d6e070ac088347f6827327d6d9e2f9630205c4fdc8",
        ["0x1.e1dcebbf8bdbcp+9", "0x1.c676ac7be2788p+9", "0x1.b663f43a9632ap+5", "0x1.de4d2cf8f734dp-1", "0x1.54fec792761cbp+5", "0x1.84b5e84bd0ae7p+7", "0x1.80af71ac97b02p+9", "0x1.af1211290d29ap-1"]],
    "mr-regrow": [[9, 7, 64, 8, 2, 16], "b5062d9f37511e008b520a776239f0fa47df2891b7fa408ce664167589cd6a99",
        ["0x1.e517e46a097d2p+10", "0x1.2e2921c70efbep+10", "0x1.6ddd8545f5027p+9", "0x1.64b2e7f35027ap-2", "0x1.3b60674c092f5p+8", "0x1.5f243fcbb01d5p+9", "0x1.3585c484316e7p+10", "0x1.2a3bb864f08e4p+8"],
        "d5675d3ba9d64fe39de87ccd461dcbc62867ea53be10b6541861bac143a6578a",
        ["0x1.e517e46a097d2p+10", "0x1.2e2921c70efbep+10", "0x1.6ddd8545f5027p+9", "0x1.64b2e7f35027ap-2", "0x1.3b60674c092f5p+8", "0x1.5f243fcbb01d5p+9", "0x1.3585c484316e7p+10", "0x1.2a3bb864f08e4p+8"]],
    "csr": [[5, 16, 4, 0, 1, 0], "1af8cebac9dd7a28f07c5048126220f86dcb857bbcf16f7f55df6ba8e8de7b52",
        ["0x1.a3cf0dca6abf8p+4", "0x1.dc6ccc2908bfap+3", "0x1.6b314f6bccbf5p+3", "0x1.5fdd22d740c38p-2", "0x1.7eb49354e4adap+2", "0x1.baa3c4113c402p+3", "0x1.8cfa5783993edp+3", "0x1.7d699ec067b85p+2"],
        "91f5009cdf23438f497f39bf6bac4d2e137816d4d84197161d7ddae38e46df7d",
        ["0x1.a3cf0dca6abf8p+4", "0x1.dc6ccc2908bfap+3", "0x1.6b314f6bccbf5p+3", "0x1.5fdd22d740c38p-2", "0x1.7eb49354e4adap+2", "0x1.baa3c4113c402p+3", "0x1.8cfa5783993edp+3", "0x1.7d699ec067b85p+2"]],
    "csr-split": [[5, 64, 4, 1, 1, 0], "65ee97febb8da637c7d55481cde5f77859561990ec1db0129f8960a8599fade9",
        ["0x1.3c0581607ff28p+5", "0x1.118d88888da09p+4", "0x1.667d7a3872448p+4", "0x1.2e59d46560998p-2", "0x1.aced05c84a3e6p+3", "0x1.3fd76d875cb17p+4", "0x1.38339539a333ap+4", "0x1.3db32c2e49977p+3"],
        "006857ec78dbe0bc407181edeb5ee814070cdf6603da7ae9eb8d0062905ea603",
        ["0x1.3c0581607ff28p+5", "0x1.118d88888da09p+4", "0x1.667d7a3872448p+4", "0x1.2e59d46560998p-2", "0x1.aced05c84a3e6p+3", "0x1.3fd76d875cb17p+4", "0x1.38339539a333ap+4", "0x1.3db32c2e49977p+3"]],
    "csr-k3": [[5, 64, 4, 1, 3, 0], "05265fea49a5cc5e46f5f57cc38e0a4c86a8e65bb9c1a63cb5aac4e00844d7ff",
        ["0x1.c6ee44654cf3cp+5", "0x1.ea7de81886904p+4", "0x1.a35ea0b213573p+4", "0x1.8e3a4e7a23045p-2", "0x1.05bb15f697523p+3", "0x1.b92f38d51d0c9p+4", "0x1.d4ad4ff57cdaep+4", "0x1.498555513881bp+3"],
        "1667867f5f5f343b8122a7030b4f0f236b6529d8a1b0160b1465fbc0a27980c3",
        ["0x1.c6ee44654cf3cp+5", "0x1.ea7de81886904p+4", "0x1.a35ea0b213573p+4", "0x1.8e3a4e7a23045p-2", "0x1.05bb15f697523p+3", "0x1.b92f38d51d0c9p+4", "0x1.d4ad4ff57cdaep+4", "0x1.498555513881bp+3"]],
    "csr-rem": [[5, 4, 64, 1, 1, 0], "d0cab95d78d9f14a8ff88579b28854ea92417d979e311f8d407e0e24fd70da23",
        ["0x1.1f4194acb0628p+8", "0x1.1f26a4fee9d64p+8", "0x1.aefadc68c36e3p-4", "0x1.ffd4bb7b665bbp-1", "0x1.efc47fb9620d4p+4", "0x1.c1e062b954265p+5", "0x1.ce0b10ab0bbb6p+7", "0x1.9b3c211dd172ap-18"],
        "783d5945624b27a5872e4a27b38196f6e4f9cebc848e50744ede5ceb0b92a7d1",
        ["0x1.1f4194acb0628p+8", "0x1.1f26a4fee9d64p+8", "0x1.aefadc68c36e3p-4", "0x1.ffd4bb7b665bbp-1", "0x1.efc47fb9620d4p+4", "0x1.c1e062b954265p+5", "0x1.ce0b10ab0bbb6p+7", "0x1.9b3c211dd172ap-18"]],
}
# ids whose live and standalone gap were byte-equal at the parent
LIVE_EQUALS_ALONE = set(TABLE)


@functools.lru_cache(maxsize=None)
def _data(name):
    """The arrays of an id - read-only, shared."""
    kind, shape, K, seed, _ = TABLE[name]
    if kind.startswith("csr"):
        A, b, lam = S.make_sparse(*shape)
        if K > 1:   # K right-hand sides of the same construction
            rng = np.random.default_rng(seed)
            X = np.zeros((A.shape[1], K))
            X[:20] = rng.standard_normal((20, K))
            b = A @ X + 0.01 * rng.standard_normal((A.shape[0], K))
            lam = 0.1 * np.max(np.abs(A.T @ b))
        return A, b, float(lam)
    A, B, lam = M.make("logistic" if kind == "logistic" else "square", shape[0], shape[1], K, seed)
    return A, (B if K > 1 else np.ascontiguousarray(B[:, 0])), lam


def _problem(name):
    from zfista_amd import problems as Z

    kind, _, K, _, _ = TABLE[name]
    A, b, lam = _data(name)
    if kind == "ls":
        return Z.LeastSquaresL1(A, b, lam)
    if kind == "logistic":
        return Z.LogisticL1(A, b, lam)
    if kind == "f32":
        return Z.LeastSquaresL1(A, b, lam, matrix_dtype="float32")
    if kind == "mr":
        return Z.MultiResponseLeastSquaresL1(A, b, lam)
    return Z.SparseMultiResponseLeastSquaresL1(A, b, lam) if K > 1 else Z.SparseLeastSquaresL1(A, b, lam)


def _hex(v):
    return [float(t).hex() for t in np.asarray(v, dtype=np.float64)[:8]]


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(np.asarray(a, dtype=np.float64)).tobytes()).hexdigest()


def fingerprint(name, setenv):
    """[ls_plan (6), sha256(x_12), live gap, sha256(jac_f(x_12)), standalone gap]; `setenv(key, value)` sets the id's environment
    before the solver is created (the library reads it once per solver)."""
    import ctypes as C

    from zfista_amd import _lib
    from zfista_amd.problems import DualityGap
    from zfista_amd.proximal_gradient import NativeRun

    kind, _, _, _, env = TABLE[name]
    for k, v in env.items():
        setenv(k, v)
    prob = _problem(name)
    opts = dict(OPTS, acceptance="remainder") if kind == "csr-rem" else OPTS
    run = NativeRun(prob, np.zeros(prob.n_features), opts)
    plan = np.zeros(6, dtype=np.int64)
    _lib.check(run.solver.lib.zf_solver_ls_plan(run.solver.handle, C.c_void_p(_lib.ptr(plan)), plan.size))
    while run.status == _lib.ZF_RUNNING:
        run.advance(4)
    assert run.status == _lib.ZF_MAXITER and run.nit_seen == 12
    x = run.solver.get_x()
    live = run.solver.duality_gap()
    run.solver.close()
    alone = prob.duality_gap(x)
    alone = [getattr(alone, k) for k in DualityGap.__slots__[:8]]
    return [[int(v) for v in plan], _sha(x), _hex(live), _sha(prob.jac_f(x)), _hex(alone)]


@pytest.mark.parametrize("name", list(TABLE))
def test_a_solve_on_each_branch_of_the_sweep_launchers_computes_the_parent_librarys_bits(name, monkeypatch):
    """Plan, x_12, the live certificate, jac_f(x_12) and the standalone certificate of the id equal what the parent commit's
    library gave; the live certificate is the standalone one byte for byte; the two regrow ids regrew their slab."""
    got = fingerprint(name, monkeypatch.setenv)
    print(name, json.dumps(got))
    if name in LIVE_EQUALS_ALONE:
        assert got[2] == got[4], "the live gap is the standalone gap, byte for byte"
    if name in REGROW:   # (after: the parent's record; before: the fp64 rule on the flattened shape zf_solver_create plans on)
        A, b, _ = _data(name)
        K = b.size // A.shape[0]
        before = M.slices_of(A.shape[0] * K, A.shape[1] * K)[0]
        assert (before, PARENT[name][0][2]) == REGROW[name] and got[0][2] == PARENT[name][0][2]
    assert got == PARENT[name]
