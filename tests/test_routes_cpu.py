"""The route table of csrc/routes.h, checked without a GPU: tests/native/routes_check.cpp fills
DProblem / RowsArgs by hand and prints which kernel instance row_route / mlp_route pick and how
vary_rows_per_wg chunks the rows; the lines must equal EXPECTED.

EXPECTED was printed by this program on the commit that moved the launchers' own conditions
into routes.h unchanged, so it records what launch_gen / launch_cons / launch_mlp did before
they consumed the route.  A change to a line is a change of product routing (or of a
development switch) and needs its own reason; the GPU route tests
(tests/test_gpu_classifier_routes.py, test_gpu_parity.py) trust the kind this table pins.

Columns: mlp kind = mv_get_mlp_kernel (-1 none, 0 k_mlp, 1 / 2 k_mlp2 genes / ML rows, 4 k_mlpw,
5 k_mlpw32, 6 / 7 k_mlpr genes / ML rows); row kind = mv_get_row_kernel (0 k_gen + k_cons,
1 k_narrow, 2 k_genc); cons = 0 none, 1 k_cons, 2 k_cons<FULL>, 3 k_consx.

What the table shows beyond the routes the GPU tests run:
  * k_mlp (kind 0) is product-reachable: fp32 nets whose k_mlpw32 tile passes the CU's 160 KiB
    (512-wide with Dm4 >= 624 or 640, by the final layer's size) and bf16 nets past k_mlpw's
    LDS.  (The lines with hidden widths that are no multiple of 16 or above 512, or with more
    than 8 classes, show mlp_route alone: mv_engine_create refuses those nets.)
  * Dm4 % 16 != 0 cannot occur (Dm4 is Dm rounded up to 16 where the problem is created).
  * 48 states of 100 offspring on 256 CUs run 960 workgroups of 5 rows (1,200 of 4 on 304).

The "mlp synth" lines are the classifier-fallback cases of tests/synth_problem.py MLP_CASES
(tests/test_gpu_mlp_fallback.py, tests/test_gpu_bf16_routes.py; tests/test_mlp_orders_cpu.py
checks each line against its case): the k_mlp<MAXCT, BF> instance each case names, in the fp32
and the bf16 mode and under MV_MLP_V1 (m639t: with MV_MLPR=0).  The MV_MLP_V1 and MV_MLPW lines
are problems whose fp32 ML rows are written (xml_direct 0), as mv_engine_create makes them under
those switches: the kernels they select read the rows, never the genes.  The "lds" lines give the three budgets at both sides
of each edge the cases sit at: k_mlpw32 fits a 512-512-2 net at Dm4 608 and not at 624;
mv_engine_create accepts that net up to Dm4 720, 512-272-3 up to 736 and 144-240-3 up to 1008;
on botnet (Dm4 432) a 512-wide last hidden layer with 8 classes puts the bf16 mode past k_mlpw.

The "row synth" lines are the synthetic shapes of tests/synth_problem.py, one per GPU case of
tests/test_gpu_row_routes.py ("/sbx": the case's second run).  The name gives the attack's
problem -- stored genes V, Dm4, C, i(dent), f(ull_ops), sd = ABS_SUMDIFF columns, c(ompact),
s(lim), x = SBX -- and mlp= the classifier kind under the cases' D-32-16-2 net: they pin the
NT / NV / FULL / SLIM instance the kind reported on the GPU does not show
(tests/test_synth_problem_cpu.py checks each line against the shape the builder makes).
The x cases carry MV_OP_EXPR columns (f2): cons=3 with nt / ident is the k_consx<IDENT, NT>
instance, all ten of them.
"""
import os
import shutil
import subprocess

import pytest

EXPECTED = """\
mlp botnet 312-64-64-32-2              kind=6 rw=1 no=2 xml=0 cj=0 bf=0 direct=0 co=0 maxct=0
mlp botnet 312-64-64-32-3              kind=6 rw=1 no=8 xml=0 cj=0 bf=0 direct=0 co=0 maxct=0
mlp botnet 432-64-64-32-2              kind=6 rw=1 no=2 xml=0 cj=0 bf=0 direct=0 co=0 maxct=0
mlp botnet odd Dm 431-64-32-2          kind=1 rw=0 no=0 xml=0 cj=1 bf=0 direct=1 co=0 maxct=0
mlp lcld 64-32-2 (ML rows)             kind=7 rw=1 no=2 xml=1 cj=0 bf=0 direct=0 co=0 maxct=0
mlp lcld 64-32-3 (ML rows)             kind=7 rw=1 no=8 xml=1 cj=0 bf=0 direct=0 co=0 maxct=0
mlp botnet hidden 80 (genes, even Dm)  kind=1 rw=0 no=0 xml=0 cj=2 bf=0 direct=1 co=1 maxct=0
mlp botnet hidden 128 (genes)          kind=1 rw=0 no=0 xml=0 cj=2 bf=0 direct=1 co=1 maxct=0
mlp botnet hidden 80 (genes, odd Dm)   kind=1 rw=0 no=0 xml=0 cj=2 bf=0 direct=1 co=0 maxct=0
mlp lcld hidden 80 (ML rows)           kind=2 rw=0 no=0 xml=0 cj=2 bf=0 direct=0 co=0 maxct=0
mlp lcld hidden 128 (ML rows)          kind=2 rw=0 no=0 xml=0 cj=2 bf=0 direct=0 co=0 maxct=0
mlp bf16 hidden 64                     kind=1 rw=0 no=0 xml=0 cj=1 bf=1 direct=1 co=0 maxct=0
mlp bf16 hidden 128                    kind=1 rw=0 no=0 xml=0 cj=2 bf=1 direct=1 co=0 maxct=0
mlp bf16 hidden 256                    kind=4 rw=0 no=0 xml=0 cj=2 bf=0 direct=0 co=0 maxct=0
mlp bf16 hidden 512                    kind=4 rw=0 no=0 xml=0 cj=4 bf=0 direct=0 co=0 maxct=0
mlp fp32 hidden 144                    kind=5 rw=0 no=0 xml=0 cj=2 bf=0 direct=0 co=0 maxct=0
mlp fp32 hidden 256                    kind=5 rw=0 no=0 xml=0 cj=2 bf=0 direct=0 co=0 maxct=0
mlp fp32 hidden 512                    kind=5 rw=0 no=0 xml=0 cj=4 bf=0 direct=0 co=0 maxct=0
mlp fp32 512 wide, 8 classes, Dm4 432  kind=5 rw=0 no=0 xml=0 cj=4 bf=0 direct=0 co=0 maxct=0
mlp fp32 hidden 512, Dm4 624           kind=5 rw=0 no=0 xml=0 cj=4 bf=0 direct=0 co=0 maxct=0
mlp fp32 hidden 512, Dm4 640           kind=0 rw=0 no=0 xml=0 cj=0 bf=0 direct=0 co=0 maxct=8
mlp bf16 hidden 512, Dm4 640           kind=0 rw=0 no=0 xml=0 cj=0 bf=1 direct=0 co=0 maxct=8
mlp fp32 hidden 520 (not 16 k)         kind=0 rw=0 no=0 xml=0 cj=0 bf=0 direct=0 co=0 maxct=8
mlp fp32 hidden 200 (not 16 k)         kind=0 rw=0 no=0 xml=0 cj=0 bf=0 direct=0 co=0 maxct=4
mlp fp32 hidden 528 (> 512)            kind=0 rw=0 no=0 xml=0 cj=0 bf=0 direct=0 co=0 maxct=8
mlp fp32 9 classes, hidden 256         kind=0 rw=0 no=0 xml=0 cj=0 bf=0 direct=0 co=0 maxct=4
mlp fp32 9 classes, hidden 64          kind=1 rw=0 no=0 xml=0 cj=1 bf=0 direct=1 co=1 maxct=0
mlp one Dense layer                    kind=1 rw=0 no=0 xml=0 cj=1 bf=0 direct=1 co=1 maxct=0
mlp no model                           kind=-1 rw=0 no=0 xml=0 cj=0 bf=0 direct=0 co=0 maxct=0
mlp MV_MLPR=0 botnet 312-64-64-32-2    kind=1 rw=0 no=0 xml=0 cj=1 bf=0 direct=1 co=1 maxct=0
mlp MV_MLPR=0 lcld 64-32-2             kind=2 rw=0 no=0 xml=0 cj=1 bf=0 direct=0 co=0 maxct=0
mlp MV_MLPR_RW=2 botnet 312-64-64-32-2 kind=6 rw=2 no=2 xml=0 cj=0 bf=0 direct=0 co=0 maxct=0
mlp MV_MLPR_RW=2 botnet ... 3 classes  kind=6 rw=2 no=8 xml=0 cj=0 bf=0 direct=0 co=0 maxct=0
mlp MV_MLPR_RW=2 lcld 64-32-2          kind=7 rw=1 no=2 xml=1 cj=0 bf=0 direct=0 co=0 maxct=0
mlp MV_MLPR_RW=7 botnet 312-64-64-32-2 kind=6 rw=2 no=2 xml=0 cj=0 bf=0 direct=0 co=0 maxct=0
mlp MV_MLP_V1 botnet hidden 128        kind=5 rw=0 no=0 xml=0 cj=1 bf=0 direct=0 co=0 maxct=0
mlp MV_MLP_V1 botnet 312-64-64-32-2    kind=7 rw=1 no=2 xml=1 cj=0 bf=0 direct=0 co=0 maxct=0
mlp MV_MLP_V1 bf16 hidden 128          kind=4 rw=0 no=0 xml=0 cj=1 bf=0 direct=0 co=0 maxct=0
mlp MV_MLPW bf16 hidden 64             kind=4 rw=0 no=0 xml=0 cj=1 bf=0 direct=0 co=0 maxct=0
mlp MV_MLPW fp32 hidden 128            kind=2 rw=0 no=0 xml=0 cj=2 bf=0 direct=0 co=0 maxct=0
mlp MV_MLPW_OFF bf16 hidden 256        kind=0 rw=0 no=0 xml=0 cj=0 bf=1 direct=0 co=0 maxct=4
mlp MV_MLPW_OFF bf16 hidden 64         kind=1 rw=0 no=0 xml=0 cj=1 bf=1 direct=1 co=0 maxct=0
mlp MV_MLPW32=0 fp32 hidden 144        kind=0 rw=0 no=0 xml=0 cj=0 bf=0 direct=0 co=0 maxct=4
mlp MV_MLPW32=0 fp32 hidden 512        kind=0 rw=0 no=0 xml=0 cj=0 bf=0 direct=0 co=0 maxct=8
mlp MV_MLP_CO=0 botnet hidden 80       kind=1 rw=0 no=0 xml=0 cj=2 bf=0 direct=1 co=0 maxct=0
mlp synth m608w Dm4 608 512-512-2 fp32 kind=5 rw=0 no=0 xml=0 cj=4 bf=0 direct=0 co=0 maxct=0
mlp synth m609w Dm4 624 512-512-2 fp32 kind=0 rw=0 no=0 xml=0 cj=0 bf=0 direct=0 co=0 maxct=8
mlp synth m609w Dm4 624 512-512-2 bf16 kind=0 rw=0 no=0 xml=0 cj=0 bf=1 direct=0 co=0 maxct=8
mlp synth m736w Dm4 736 512-272-3 fp32 kind=0 rw=0 no=0 xml=0 cj=0 bf=0 direct=0 co=0 maxct=8
mlp synth m1008w Dm4 1008 144-240-3 fp32 kind=0 rw=0 no=0 xml=0 cj=0 bf=0 direct=0 co=0 maxct=4
mlp synth m1008w Dm4 1008 144-240-3 bf16 kind=0 rw=0 no=0 xml=0 cj=0 bf=1 direct=0 co=0 maxct=4
mlp synth m640n Dm4 640 48-80-2 fp32   kind=1 rw=0 no=0 xml=0 cj=2 bf=0 direct=1 co=1 maxct=0
mlp synth m640n Dm4 640 48-80-2 fp32 MV_MLP_V1 kind=0 rw=0 no=0 xml=0 cj=0 bf=0 direct=0 co=0 maxct=2
mlp synth m639t Dm4 640 32-16-8 fp32   kind=1 rw=0 no=0 xml=0 cj=1 bf=0 direct=1 co=0 maxct=0
mlp synth m639t Dm4 640 32-16-8 fp32 MV_MLP_V1 kind=0 rw=0 no=0 xml=0 cj=0 bf=0 direct=0 co=0 maxct=1
mlp MV_MLP_V1 even Dm 640-32-16-8      kind=7 rw=1 no=8 xml=1 cj=0 bf=0 direct=0 co=0 maxct=0
mlp bf16 botnet 756-512-512-8          kind=0 rw=0 no=0 xml=0 cj=0 bf=1 direct=0 co=0 maxct=8
mlp bf16 botnet 756-512-256-8          kind=4 rw=0 no=0 xml=0 cj=4 bf=0 direct=0 co=0 maxct=0
lds Dm4 608-512-512-2 k_mlp=147856 create=ok k_mlpw32=161040 k_mlpw=166160
lds Dm4 624-512-512-2 k_mlp=149904 create=ok k_mlpw32=165136 k_mlpw=174352
lds Dm4 720-512-512-2 k_mlp=162192 create=ok k_mlpw32=189712 k_mlpw=198928
lds Dm4 736-512-512-2 k_mlp=164240 create=refused k_mlpw32=193808 k_mlpw=198928
lds Dm4 736-512-272-3 k_mlp=163408 create=ok k_mlpw32=192976 k_mlpw=200144
lds Dm4 752-512-272-3 k_mlp=165456 create=refused k_mlpw32=197072 k_mlpw=208336
lds Dm4 1008-144-240-3 k_mlp=163024 create=ok k_mlpw32=262224 k_mlpw=273488
lds Dm4 1024-144-240-3 k_mlp=165072 create=refused k_mlpw32=266320 k_mlpw=273488
lds Dm4 432-512-512-8 k_mlp=147872 create=ok k_mlpw32=148768 k_mlpw=166176
lds Dm4 432-512-256-8 k_mlp=139680 create=ok k_mlpw32=140576 k_mlpw=157984
row botnet full layout V 432           kind=2 nt=7 ident=1 sbx=0 slim=1 cons=0 nv=0 full=0 need_plan=1 plan_missing=0
row botnet compact V 312 Vr 432        kind=2 nt=5 ident=1 sbx=0 slim=1 cons=0 nv=0 full=0 need_plan=1 plan_missing=0
row botnet SBX                         kind=2 nt=7 ident=1 sbx=1 slim=1 cons=0 nv=0 full=0 need_plan=1 plan_missing=0
row botnet slim 0                      kind=2 nt=7 ident=1 sbx=0 slim=0 cons=0 nv=0 full=0 need_plan=1 plan_missing=0
row botnet slim 0 SBX                  kind=2 nt=7 ident=1 sbx=1 slim=0 cons=0 nv=0 full=0 need_plan=1 plan_missing=0
row botnet mode 0 (genes given)        kind=2 nt=7 ident=1 sbx=0 slim=1 cons=0 nv=0 full=0 need_plan=0 plan_missing=0
row botnet mode 1 without a plan       kind=2 nt=7 ident=1 sbx=0 slim=1 cons=0 nv=0 full=0 need_plan=1 plan_missing=1
row botnet do_eval 0                   kind=0 nt=8 ident=1 sbx=0 slim=0 cons=0 nv=0 full=0 need_plan=0 plan_missing=0
row lcld V 8                           kind=1 nt=0 ident=0 sbx=0 slim=0 cons=0 nv=8 full=1 need_plan=0 plan_missing=0
row lcld V 9                           kind=1 nt=0 ident=0 sbx=0 slim=0 cons=0 nv=16 full=1 need_plan=0 plan_missing=0
row lcld V 15                          kind=1 nt=0 ident=0 sbx=0 slim=0 cons=0 nv=16 full=1 need_plan=0 plan_missing=0
row lcld V 16                          kind=1 nt=0 ident=0 sbx=0 slim=0 cons=0 nv=16 full=1 need_plan=0 plan_missing=0
row lcld V 17                          kind=1 nt=0 ident=0 sbx=0 slim=0 cons=0 nv=32 full=1 need_plan=0 plan_missing=0
row lcld V 32                          kind=1 nt=0 ident=0 sbx=0 slim=0 cons=0 nv=32 full=1 need_plan=0 plan_missing=0
row lcld V 33                          kind=0 nt=1 ident=0 sbx=0 slim=0 cons=2 nv=0 full=0 need_plan=0 plan_missing=0
row lcld V 15 without financial ops    kind=1 nt=0 ident=0 sbx=0 slim=0 cons=0 nv=16 full=0 need_plan=0 plan_missing=0
row lcld SBX                           kind=0 nt=1 ident=0 sbx=1 slim=0 cons=2 nv=0 full=0 need_plan=0 plan_missing=0
row lcld SBX, mode 0                   kind=1 nt=0 ident=0 sbx=0 slim=0 cons=0 nv=16 full=1 need_plan=0 plan_missing=0
row lcld expr columns (full_ops 2)     kind=0 nt=1 ident=0 sbx=0 slim=0 cons=3 nv=0 full=0 need_plan=0 plan_missing=0
row botnet expr columns (full_ops 2)   kind=0 nt=8 ident=1 sbx=0 slim=0 cons=3 nv=0 full=0 need_plan=0 plan_missing=0
row lcld compact                       kind=0 nt=1 ident=0 sbx=0 slim=0 cons=2 nv=0 full=0 need_plan=0 plan_missing=0
row lcld with a sum-diff op            kind=0 nt=1 ident=0 sbx=0 slim=0 cons=2 nv=0 full=0 need_plan=0 plan_missing=0
row lcld 65 ops                        kind=0 nt=1 ident=0 sbx=0 slim=0 cons=2 nv=0 full=0 need_plan=0 plan_missing=0
row lcld do_eval 0                     kind=0 nt=1 ident=0 sbx=0 slim=0 cons=0 nv=0 full=0 need_plan=0 plan_missing=0
row ident max(V, Dm4) 128              kind=0 nt=2 ident=1 sbx=0 slim=0 cons=1 nv=0 full=0 need_plan=0 plan_missing=0
row ident max(V, Dm4) 129              kind=2 nt=4 ident=1 sbx=0 slim=0 cons=0 nv=0 full=0 need_plan=1 plan_missing=0
row ident V 120 (Dm4 128)              kind=0 nt=2 ident=1 sbx=0 slim=0 cons=1 nv=0 full=0 need_plan=0 plan_missing=0
row ident V 40 (one gene per lane)     kind=0 nt=1 ident=1 sbx=0 slim=0 cons=1 nv=0 full=0 need_plan=0 plan_missing=0
row ident V 100 (two per lane)         kind=0 nt=2 ident=1 sbx=0 slim=0 cons=1 nv=0 full=0 need_plan=0 plan_missing=0
row ident V 257 (k_genc NT 5)          kind=2 nt=5 ident=1 sbx=0 slim=0 cons=0 nv=0 full=0 need_plan=1 plan_missing=0
row ident V 384 (k_genc NT 6)          kind=2 nt=6 ident=1 sbx=0 slim=0 cons=0 nv=0 full=0 need_plan=1 plan_missing=0
row ident V 512 (k_genc NT 8)          kind=2 nt=8 ident=1 sbx=0 slim=0 cons=0 nv=0 full=0 need_plan=1 plan_missing=0
row ident V 513 (k_genc NT 16)         kind=2 nt=16 ident=1 sbx=0 slim=0 cons=0 nv=0 full=0 need_plan=1 plan_missing=0
row not ident V 432                    kind=0 nt=8 ident=0 sbx=0 slim=0 cons=1 nv=0 full=0 need_plan=0 plan_missing=0
row not ident V 600                    kind=0 nt=16 ident=0 sbx=0 slim=0 cons=1 nv=0 full=0 need_plan=0 plan_missing=0
row MV_NARROW=0 lcld V 15              kind=0 nt=1 ident=0 sbx=0 slim=0 cons=2 nv=0 full=0 need_plan=0 plan_missing=0
row MV_NARROW=0 botnet                 kind=2 nt=7 ident=1 sbx=0 slim=1 cons=0 nv=0 full=0 need_plan=1 plan_missing=0
row MV_GENC=0 botnet                   kind=0 nt=8 ident=1 sbx=0 slim=0 cons=1 nv=0 full=0 need_plan=0 plan_missing=0
row MV_GENC=0 botnet SBX               kind=0 nt=8 ident=1 sbx=1 slim=0 cons=1 nv=0 full=0 need_plan=0 plan_missing=0
row MV_GENC=0 lcld V 15                kind=1 nt=0 ident=0 sbx=0 slim=0 cons=0 nv=16 full=1 need_plan=0 plan_missing=0
rows_per_wg n 100, 387 states          rows=20 chunks_per_state=5 workgroups=1935
rows_per_wg n 203, 387 states          rows=23 chunks_per_state=9 workgroups=3483
rows_per_wg n 100, 48 states           rows=5 chunks_per_state=20 workgroups=960
rows_per_wg n 100, 12 states           rows=4 chunks_per_state=25 workgroups=300
rows_per_wg n 100, 1 state             rows=4 chunks_per_state=25 workgroups=25
rows_per_wg n 3, 387 states            rows=3 chunks_per_state=1 workgroups=387
rows_per_wg n 3, 1 state               rows=3 chunks_per_state=1 workgroups=1
rows_per_wg n 100, states unknown      rows=20 chunks_per_state=5 workgroups=5
rows_per_wg n 100, 48 states, 304 CUs  rows=4 chunks_per_state=25 workgroups=1200
rows_per_wg n 100, 48 states, cap 16   rows=15 chunks_per_state=7 workgroups=336
rows_per_wg n 100, 387 states, cap 64  rows=25 chunks_per_state=4 workgroups=1548
rows_per_wg n 100, 387 states, cap 1   rows=4 chunks_per_state=25 workgroups=9675
row synth n8p V8 Dm4 16 C5 i1 f0 sd0 c0 s0 x0 kind=1 nt=0 ident=0 sbx=0 slim=0 cons=0 nv=8 full=0 need_plan=0 plan_missing=0 mlp=6
row synth n8p/sbx V8 Dm4 16 C5 i1 f0 sd0 c0 s0 x1 kind=0 nt=1 ident=1 sbx=1 slim=0 cons=1 nv=0 full=0 need_plan=0 plan_missing=0 mlp=6
row synth n8f V8 Dm4 16 C8 i0 f1 sd0 c0 s0 x0 kind=1 nt=0 ident=0 sbx=0 slim=0 cons=0 nv=8 full=1 need_plan=0 plan_missing=0 mlp=7
row synth n9 V9 Dm4 16 C6 i1 f0 sd0 c0 s0 x0 kind=1 nt=0 ident=0 sbx=0 slim=0 cons=0 nv=16 full=0 need_plan=0 plan_missing=0 mlp=1
row synth n16f V16 Dm4 32 C10 i0 f1 sd0 c0 s0 x0 kind=1 nt=0 ident=0 sbx=0 slim=0 cons=0 nv=16 full=1 need_plan=0 plan_missing=0 mlp=7
row synth n17f V17 Dm4 32 C10 i0 f1 sd0 c0 s0 x0 kind=1 nt=0 ident=0 sbx=0 slim=0 cons=0 nv=32 full=1 need_plan=0 plan_missing=0 mlp=7
row synth n32 V32 Dm4 64 C64 i0 f0 sd0 c0 s0 x0 kind=1 nt=0 ident=0 sbx=0 slim=0 cons=0 nv=32 full=0 need_plan=0 plan_missing=0 mlp=7
row synth n32d V32 Dm4 80 C64 i0 f0 sd0 c0 s0 x0 kind=0 nt=2 ident=0 sbx=0 slim=0 cons=1 nv=0 full=0 need_plan=0 plan_missing=0 mlp=7
row synth n32c V32 Dm4 64 C65 i0 f0 sd0 c0 s0 x0 kind=0 nt=1 ident=0 sbx=0 slim=0 cons=1 nv=0 full=0 need_plan=0 plan_missing=0 mlp=7
row synth n8s V8 Dm4 16 C6 i1 f0 sd1 c0 s0 x0 kind=0 nt=1 ident=1 sbx=0 slim=0 cons=1 nv=0 full=0 need_plan=0 plan_missing=0 mlp=6
row synth n2 V2 Dm4 16 C2 i1 f0 sd0 c0 s1 x0 kind=1 nt=0 ident=0 sbx=0 slim=0 cons=0 nv=8 full=0 need_plan=0 plan_missing=0 mlp=6
row synth g33 V33 Dm4 48 C20 i1 f0 sd0 c0 s0 x0 kind=0 nt=1 ident=1 sbx=0 slim=0 cons=1 nv=0 full=0 need_plan=0 plan_missing=0 mlp=1
row synth g33/sbx V33 Dm4 48 C20 i1 f0 sd0 c0 s0 x1 kind=0 nt=1 ident=1 sbx=1 slim=0 cons=1 nv=0 full=0 need_plan=0 plan_missing=0 mlp=1
row synth g64 V64 Dm4 64 C40 i1 f0 sd0 c0 s0 x0 kind=0 nt=1 ident=1 sbx=0 slim=0 cons=1 nv=0 full=0 need_plan=0 plan_missing=0 mlp=6
row synth g65 V65 Dm4 80 C40 i1 f0 sd0 c0 s0 x0 kind=0 nt=2 ident=1 sbx=0 slim=0 cons=1 nv=0 full=0 need_plan=0 plan_missing=0 mlp=1
row synth g65/sbx V65 Dm4 80 C40 i1 f0 sd0 c0 s0 x1 kind=0 nt=2 ident=1 sbx=1 slim=0 cons=1 nv=0 full=0 need_plan=0 plan_missing=0 mlp=1
row synth g128 V128 Dm4 128 C70 i1 f0 sd0 c0 s0 x0 kind=0 nt=2 ident=1 sbx=0 slim=0 cons=1 nv=0 full=0 need_plan=0 plan_missing=0 mlp=6
row synth o40f V40 Dm4 64 C24 i0 f1 sd0 c0 s0 x0 kind=0 nt=1 ident=0 sbx=0 slim=0 cons=2 nv=0 full=0 need_plan=0 plan_missing=0 mlp=7
row synth o100p V100 Dm4 160 C70 i0 f0 sd0 c0 s0 x0 kind=0 nt=4 ident=0 sbx=0 slim=0 cons=1 nv=0 full=0 need_plan=0 plan_missing=0 mlp=7
row synth o100p/sbx V100 Dm4 160 C70 i0 f0 sd0 c0 s0 x1 kind=0 nt=4 ident=0 sbx=1 slim=0 cons=1 nv=0 full=0 need_plan=0 plan_missing=0 mlp=7
row synth o300f V300 Dm4 336 C100 i0 f1 sd0 c0 s0 x0 kind=0 nt=8 ident=0 sbx=0 slim=0 cons=2 nv=0 full=0 need_plan=0 plan_missing=0 mlp=7
row synth o520p V520 Dm4 608 C150 i0 f0 sd0 c0 s0 x0 kind=0 nt=16 ident=0 sbx=0 slim=0 cons=1 nv=0 full=0 need_plan=0 plan_missing=0 mlp=7
row synth c129 V129 Dm4 144 C70 i1 f0 sd0 c0 s1 x0 kind=2 nt=4 ident=1 sbx=0 slim=1 cons=0 nv=0 full=0 need_plan=1 plan_missing=0 mlp=1
row synth c129/sbx V129 Dm4 144 C70 i1 f0 sd0 c0 s1 x1 kind=2 nt=4 ident=1 sbx=1 slim=1 cons=0 nv=0 full=0 need_plan=1 plan_missing=0 mlp=1
row synth c256 V256 Dm4 256 C100 i1 f0 sd0 c0 s1 x0 kind=2 nt=4 ident=1 sbx=0 slim=1 cons=0 nv=0 full=0 need_plan=1 plan_missing=0 mlp=6
row synth c257 V257 Dm4 272 C100 i1 f0 sd0 c0 s1 x0 kind=2 nt=5 ident=1 sbx=0 slim=1 cons=0 nv=0 full=0 need_plan=1 plan_missing=0 mlp=1
row synth c384 V384 Dm4 384 C130 i1 f0 sd0 c0 s1 x0 kind=2 nt=6 ident=1 sbx=0 slim=1 cons=0 nv=0 full=0 need_plan=1 plan_missing=0 mlp=6
row synth c384/sbx V384 Dm4 384 C130 i1 f0 sd0 c0 s1 x1 kind=2 nt=6 ident=1 sbx=1 slim=1 cons=0 nv=0 full=0 need_plan=1 plan_missing=0 mlp=6
row synth c385 V385 Dm4 400 C130 i1 f0 sd0 c0 s1 x0 kind=2 nt=7 ident=1 sbx=0 slim=1 cons=0 nv=0 full=0 need_plan=1 plan_missing=0 mlp=1
row synth c512 V512 Dm4 512 C150 i1 f0 sd0 c0 s1 x0 kind=2 nt=8 ident=1 sbx=0 slim=1 cons=0 nv=0 full=0 need_plan=1 plan_missing=0 mlp=6
row synth c513 V513 Dm4 528 C150 i1 f0 sd0 c0 s1 x0 kind=2 nt=16 ident=1 sbx=0 slim=1 cons=0 nv=0 full=0 need_plan=1 plan_missing=0 mlp=1
row synth c1024 V1024 Dm4 1024 C300 i1 f0 sd0 c0 s1 x0 kind=2 nt=16 ident=1 sbx=0 slim=1 cons=0 nv=0 full=0 need_plan=1 plan_missing=0 mlp=6
row synth c300x V300 Dm4 304 C400 i1 f0 sd0 c0 s0 x0 kind=2 nt=5 ident=1 sbx=0 slim=0 cons=0 nv=0 full=0 need_plan=1 plan_missing=0 mlp=6
row synth c300d V300 Dm4 304 C100 i1 f0 sd3 c0 s1 x0 kind=2 nt=5 ident=1 sbx=0 slim=1 cons=0 nv=0 full=0 need_plan=1 plan_missing=0 mlp=6
row synth k_slab V136 Dm4 144 C80 i1 f0 sd0 c1 s1 x0 kind=2 nt=4 ident=1 sbx=0 slim=1 cons=0 nv=0 full=0 need_plan=1 plan_missing=0 mlp=6
row synth k_last V199 Dm4 208 C80 i1 f0 sd0 c1 s1 x0 kind=2 nt=4 ident=1 sbx=0 slim=1 cons=0 nv=0 full=0 need_plan=1 plan_missing=0 mlp=1
row synth k_odd V143 Dm4 144 C80 i1 f0 sd0 c1 s1 x0 kind=2 nt=4 ident=1 sbx=0 slim=1 cons=0 nv=0 full=0 need_plan=1 plan_missing=0 mlp=1
row synth k_few V3 Dm4 16 C80 i1 f0 sd0 c1 s1 x0 kind=0 nt=1 ident=1 sbx=0 slim=0 cons=1 nv=0 full=0 need_plan=0 plan_missing=0 mlp=1
row synth k_mixed V160 Dm4 160 C80 i1 f0 sd0 c1 s1 x0 kind=2 nt=4 ident=1 sbx=0 slim=1 cons=0 nv=0 full=0 need_plan=1 plan_missing=0 mlp=6
row synth x64 V64 Dm4 64 C40 i1 f2 sd0 c0 s0 x0 kind=0 nt=1 ident=1 sbx=0 slim=0 cons=3 nv=0 full=0 need_plan=0 plan_missing=0 mlp=6
row synth x65 V65 Dm4 80 C40 i1 f2 sd0 c0 s0 x0 kind=0 nt=2 ident=1 sbx=0 slim=0 cons=3 nv=0 full=0 need_plan=0 plan_missing=0 mlp=1
row synth x65/sbx V65 Dm4 80 C40 i1 f2 sd0 c0 s0 x1 kind=0 nt=2 ident=1 sbx=1 slim=0 cons=3 nv=0 full=0 need_plan=0 plan_missing=0 mlp=1
row synth x128 V128 Dm4 128 C70 i1 f2 sd0 c0 s0 x0 kind=0 nt=2 ident=1 sbx=0 slim=0 cons=3 nv=0 full=0 need_plan=0 plan_missing=0 mlp=6
row synth x129 V129 Dm4 144 C70 i1 f2 sd0 c0 s0 x0 kind=0 nt=4 ident=1 sbx=0 slim=0 cons=3 nv=0 full=0 need_plan=0 plan_missing=0 mlp=1
row synth x256 V256 Dm4 256 C100 i1 f2 sd0 c0 s0 x0 kind=0 nt=4 ident=1 sbx=0 slim=0 cons=3 nv=0 full=0 need_plan=0 plan_missing=0 mlp=6
row synth x257 V257 Dm4 272 C100 i1 f2 sd0 c0 s0 x0 kind=0 nt=8 ident=1 sbx=0 slim=0 cons=3 nv=0 full=0 need_plan=0 plan_missing=0 mlp=1
row synth x512 V512 Dm4 512 C150 i1 f2 sd0 c0 s0 x0 kind=0 nt=8 ident=1 sbx=0 slim=0 cons=3 nv=0 full=0 need_plan=0 plan_missing=0 mlp=6
row synth x513 V513 Dm4 528 C150 i1 f2 sd0 c0 s0 x0 kind=0 nt=16 ident=1 sbx=0 slim=0 cons=3 nv=0 full=0 need_plan=0 plan_missing=0 mlp=1
row synth x1024 V1024 Dm4 1024 C300 i1 f2 sd0 c0 s0 x0 kind=0 nt=16 ident=1 sbx=0 slim=0 cons=3 nv=0 full=0 need_plan=0 plan_missing=0 mlp=6
row synth x300c V300 Dm4 304 C400 i1 f2 sd3 c0 s0 x0 kind=0 nt=8 ident=1 sbx=0 slim=0 cons=3 nv=0 full=0 need_plan=0 plan_missing=0 mlp=6
row synth xo32d V32 Dm4 80 C64 i0 f2 sd0 c0 s0 x0 kind=0 nt=2 ident=0 sbx=0 slim=0 cons=3 nv=0 full=0 need_plan=0 plan_missing=0 mlp=7
row synth xo100 V100 Dm4 160 C70 i0 f2 sd0 c0 s0 x0 kind=0 nt=4 ident=0 sbx=0 slim=0 cons=3 nv=0 full=0 need_plan=0 plan_missing=0 mlp=7
row synth xo100/sbx V100 Dm4 160 C70 i0 f2 sd0 c0 s0 x1 kind=0 nt=4 ident=0 sbx=1 slim=0 cons=3 nv=0 full=0 need_plan=0 plan_missing=0 mlp=7
row synth xo300f V300 Dm4 336 C100 i0 f2 sd0 c0 s0 x0 kind=0 nt=8 ident=0 sbx=0 slim=0 cons=3 nv=0 full=0 need_plan=0 plan_missing=0 mlp=7
row synth xo520 V520 Dm4 608 C150 i0 f2 sd0 c0 s0 x0 kind=0 nt=16 ident=0 sbx=0 slim=0 cons=3 nv=0 full=0 need_plan=0 plan_missing=0 mlp=7
row synth xn8f V8 Dm4 16 C8 i0 f2 sd0 c0 s0 x0 kind=0 nt=1 ident=0 sbx=0 slim=0 cons=3 nv=0 full=0 need_plan=0 plan_missing=0 mlp=7
row synth xk_last V199 Dm4 208 C80 i1 f2 sd0 c1 s0 x0 kind=0 nt=4 ident=1 sbx=0 slim=0 cons=3 nv=0 full=0 need_plan=0 plan_missing=0 mlp=1
row synth xk_odd V143 Dm4 144 C80 i1 f2 sd0 c1 s0 x0 kind=0 nt=4 ident=1 sbx=0 slim=0 cons=3 nv=0 full=0 need_plan=0 plan_missing=0 mlp=1
row synth xk_few V3 Dm4 16 C80 i1 f2 sd0 c1 s0 x0 kind=0 nt=1 ident=1 sbx=0 slim=0 cons=3 nv=0 full=0 need_plan=0 plan_missing=0 mlp=1
row synth xk_mixed V160 Dm4 160 C80 i1 f2 sd0 c1 s0 x0 kind=0 nt=4 ident=1 sbx=0 slim=0 cons=3 nv=0 full=0 need_plan=0 plan_missing=0 mlp=6
"""


def test_route_table(tmp_path):
    cxx = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(cxx):
        pytest.skip("hipcc not found")
    here = os.path.dirname(os.path.abspath(__file__))
    csrc = os.path.join(os.path.dirname(here), "moeva2-ijcai22-replication_amd", "csrc")
    exe = str(tmp_path / "routes_check")
    subprocess.run([cxx, "-O2", "-std=c++17", "-I", csrc,
                    os.path.join(here, "native", "routes_check.cpp"), "-o", exe],
                   check=True, capture_output=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    got, want = r.stdout.splitlines(), EXPECTED.splitlines()
    diff = [f"- {w}\n+ {g}" for w, g in zip(want, got) if w != g]
    assert not diff and len(got) == len(want), "\n".join(diff) or (len(got), len(want))
