"""K1 .. K3 and the vertex-map filters on crafted scans, CPU side: pins the oracle (oracle/o_preprocess.c) against a plain
fp64 statement of Preprocessing::process (tests/preprocess_ref.py), proves each structural row's property, and fixes the
inputs that tests/test_gpu_preprocess_crafted.py runs through k_preprocess.hip and k_filters.hip.

A. Room scenes against fp64 (ROOM_IDS): k6_ref's analytic room (planes x = +-5, y = +-5, floor, ceiling) seen from the
   origin at 48 x 12, 64 x 16, 333 x 10 and 70 x 9 (the last overhangs both the 64 x 8 tile of K2 + K3 and the 64 x 4 tile
   of K1c).  The points are generated FROM texels (texel_layout, room_scan): 0 .. 4 per texel in a fixed pattern, each
   0.15 .. 0.85 into its texel in both directions, ranges inside a texel at least 16 mm apart, the order shuffled by a
   fixed permutation.  Labels come in 16 x 8 blocks (edges on columns 63|64, rows 7|8) with a single-texel island, a patch
   of a dynamic class, and unlabelled gaps of 1, 3 and 5 columns; where the fill is exercised the range is a constant 6 m
   with a 1.5 % step (one side of a gap within 0.7 %, the other beyond) and 2 % spikes (every neighbour refused).  Every
   scene runs at timestamp 0 and 12, with label_offset / prob_offset at their quirk values (4 / 5: the label arrays are
   laid out so that point i still receives its texel's label), at 0, with no labels, and under the six parameter sets of
   FILTER_VARIANTS (filter0 .. filter5).

   A texel is DECIDED when every margin of every point that could reach it, and of every gate its result passes, exceeds
   a bound (preprocess_ref.py lists the margins).  The bounds are measured on the ORACLE
   (oracle/debug/o_preprocess_terms.c), never on the kernel: EPS = 2 max|oracle term - fp64 term| over the scene for the
   texel coordinates (+ one fp32 ulp of the coordinate, for the floor), the window depth, len = |un x vn| and the fill's
   |lp - lq| - 0.007 lp.  Derived from the format instead: the depth tie (a gap of 1 quantum + EPS, rounding being
   monotone), two fp32 steps of the point's own range on the clip, and the w channels (exact, test_w_channel_is_exact).
   K2 and K3 read texels up to 3 away, K1c up to 6 (+ 1 for the GL-initial fetch): a texel is decided only if those are.
   With a filter on, K2 / K3 are held against fp64 run on the vertex map of the frame under test, after that map itself
   was held against fp64's filtered map; under the blended scatter the labels are fp32 SUMS in index order, whose
   equality tests fp64 cannot decide -- they are compared with the oracle in bits only.

   Asserted on every scene: at most 2 % of the texels undecided; every outcome the parameter set allows at least 10 times
   among the decided (no label outcomes without labels or under the blended scatter; the drop only at timestamp 0; the
   three validity rules only where the fetch is NEAREST or no filter feeds K2 -- the GL-initial fetch smears the holes
   they need).  On the decided: the vertex is fp64's winner point, bit for bit; label and fill outcome exact, the
   probability within 2^-24 relative (the one division); the normal's w exact and its components within
   8 * 2^-24 * sum|terms| carried through both normalisations (preprocess_ref.normal_bound: this form fits, no measured
   bound is used); the K1b mean within n * 2^-24 * sum|terms|; the K1c range within K1C_RANGE_BOUND = 2 x 6.92e-6 m, twice
   the oracle's worst deviation over the 72 scenes (no sum-of-products form follows simply through exp and the division
   of two 169-term sums), the vertex within that + 8 * 2^-24 |component|.

   measured with the CPU oracle (EPS texel [px], window depth, len, fill [m]; undecided in %; normal: worst deviation in
   units of 2^-24 sum|terms| -- bound 8 -- and absolute; then the outcomes among the decided: empty, single, contested,
   dropped, rule 1, rule 2 (alone), rule 3 (without 1), eroded, fill at 1, fill at 2, a neighbour refused, all refused;
   last the worst K1b deviation in units of its bound, or the worst K1c range deviation in m):

       room48x12-quirk-t0         1.26e-05 4.6e-08 3.8e-07 1.6e-06  0.00  0.92 1.7e-07    36   135   405    35    28    21    82    86   125    69   100    96
       room48x12-quirk-t12        1.26e-05 4.6e-08 3.8e-07 1.6e-06  0.00  1.06 2.0e-07    36   135   405     0    24    21    66   103   153    71    84    79
       room48x12-offset0-t0       1.26e-05 4.6e-08 3.8e-07 1.6e-06  0.00  0.92 1.7e-07    36   135   405    36    27    21    84    87   123    68   100    97
       room48x12-offset0-t12      1.26e-05 4.6e-08 3.8e-07 1.6e-06  0.00  1.06 2.0e-07    36   135   405     0    24    21    66   105   152    72    83    79
       room48x12-nolabels-t0      1.26e-05 4.6e-08 3.8e-07 1.6e-06  0.00  1.06 2.0e-07    36   135   405     0    24    21    66     0     0     0     0     0
       room48x12-nolabels-t12     1.26e-05 4.6e-08 3.8e-07 1.6e-06  0.00  1.06 2.0e-07    36   135   405     0    24    21    66     0     0     0     0     0
       room48x12-filter0-t0       1.26e-05 4.6e-08 3.9e-07 1.9e-06  0.35  1.22 1.3e-07    36   135   403     -     6     2    69   192    16    13    39    37 k1b 0.25
       room48x12-filter0-t12      1.26e-05 4.6e-08 4.2e-07 1.9e-06  0.00  1.06 1.3e-07    36   135   405     -     1     2    57   203    20    15    40    38 k1b 0.25
       room48x12-filter1-t0       1.26e-05 4.6e-08 3.8e-07 1.8e-06  0.00  1.08 1.3e-07    36   135   405     -    29    21    80   170    16    16    35    34 k1b 0.27
       room48x12-filter1-t12      1.26e-05 4.6e-08 3.8e-07 1.8e-06  0.00  1.22 1.3e-07    36   135   405     -    24    21    66   203    20    20    34    33 k1b 0.27
       room48x12-filter2-t0       1.26e-05 4.6e-08 4.1e-07 1.7e-06  0.00  1.07 1.2e-07    36   135   405    35    33    25   106   100    74    42   208   188 k1c 5.02e-06
       room48x12-filter2-t12      1.26e-05 4.6e-08 3.5e-07 1.6e-06  0.00  0.96 1.2e-07    36   135   405     0    15    19    78   103   103    37   184   163 k1c 4.86e-06
       room48x12-filter3-t0       1.26e-05 4.6e-08 4.1e-07 1.7e-06  0.00  0.96 2.2e-07    36   135   405    35    28    21    82    86   129    83    79    78 k1c 3.79e-06
       room48x12-filter3-t12      1.26e-05 4.6e-08 3.6e-07 1.7e-06  0.00  1.16 5.9e-07    36   135   405     0    24    21    66   103   162    86    55    55 k1c 4.33e-06
       room48x12-filter4-t0       1.26e-05 4.6e-08 4.5e-07 1.7e-06  0.00  1.04 1.2e-07    36   135   405     -     4     3    58   203    18    12    43    43 k1c 5.41e-06
       room48x12-filter4-t12      1.26e-05 4.6e-08 4.1e-07 1.9e-06  0.00  0.99 1.2e-07    36   135   405     -     0     3    50   203    21    13    39    39 k1c 5.83e-06
       room48x12-filter5-t0       1.26e-05 4.6e-08 3.8e-07 1.6e-06  0.00  0.92 1.7e-07    36   135   405    35    28    21    82    86   125    69   100    96
       room48x12-filter5-t12      1.26e-05 4.6e-08 3.8e-07 1.6e-06  0.00  1.06 2.0e-07    36   135   405     0    24    21    66   103   153    71    84    79
       room64x16-quirk-t0         1.65e-05 4.2e-08 3.9e-07 1.9e-06  0.00  1.06 2.4e-07    64   239   721    47    45    40   134   151   237   112   168   158
       room64x16-quirk-t12        1.65e-05 4.2e-08 3.9e-07 1.9e-06  0.00  1.06 2.4e-07    64   239   721     0    44    40    96   182   278   118   140   130
       room64x16-offset0-t0       1.65e-05 4.2e-08 3.9e-07 1.9e-06  0.00  1.06 2.4e-07    64   239   721    48    44    40   136   152   236   114   168   158
       room64x16-offset0-t12      1.65e-05 4.2e-08 3.9e-07 1.9e-06  0.00  1.06 2.4e-07    64   239   721     0    44    40    96   184   278   120   140   130
       room64x16-nolabels-t0      1.65e-05 4.2e-08 3.9e-07 1.9e-06  0.00  1.06 2.4e-07    64   239   721     0    44    40    96     0     0     0     0     0
       room64x16-nolabels-t12     1.65e-05 4.2e-08 3.9e-07 1.9e-06  0.00  1.06 2.4e-07    64   239   721     0    44    40    96     0     0     0     0     0
       room64x16-filter0-t0       1.65e-05 4.2e-08 3.4e-07 1.8e-06  0.29  1.31 1.4e-07    64   239   718     -     4     2   101   346    40    22    54    52 k1b 0.22
       room64x16-filter0-t12      1.65e-05 4.2e-08 3.5e-07 1.8e-06  0.00  1.31 1.4e-07    64   239   721     -     3     2    73   363    45    25    52    50 k1b 0.22
       room64x16-filter1-t0       1.65e-05 4.2e-08 4.3e-07 1.8e-06  0.00  1.18 1.2e-07    64   239   721     -    45    40   134   319    29    18    60    59 k1b 0.29
       room64x16-filter1-t12      1.65e-05 4.2e-08 4.3e-07 1.8e-06  0.00  1.18 1.3e-07    64   239   721     -    44    40    96   363    40    24    57    56 k1b 0.29
       room64x16-filter2-t0       1.65e-05 4.2e-08 3.8e-07 1.7e-06  0.00  1.15 1.2e-07    64   239   721    47    45    45   174   174   137    55   365   330 k1c 5.30e-06
       room64x16-filter2-t12      1.65e-05 4.2e-08 4.9e-07 1.8e-06  0.00  1.11 1.3e-07    64   239   721     0    29    29   112   182   173    51   333   302 k1c 5.75e-06
       room64x16-filter3-t0       1.65e-05 4.2e-08 4.1e-07 2.0e-06  0.00  1.09 1.3e-07    64   239   721    47    45    40   134   151   250    88   172   169 k1c 6.11e-06
       room64x16-filter3-t12      1.65e-05 4.2e-08 3.9e-07 2.0e-06  0.00  1.20 4.7e-07    64   239   721     0    44    40    96   182   295    95   136   136 k1c 5.51e-06
       room64x16-filter4-t0       1.65e-05 4.2e-08 4.4e-07 1.7e-06  0.00  1.17 1.3e-07    64   239   721     -     0     3    94   363    33    20    71    67 k1c 6.58e-06
       room64x16-filter4-t12      1.65e-05 4.2e-08 3.9e-07 1.7e-06  0.00  1.03 1.3e-07    64   239   721     -     0     3    66   363    41    19    62    60 k1c 6.06e-06
       room64x16-filter5-t0       1.65e-05 4.2e-08 3.9e-07 1.9e-06  0.00  1.06 2.4e-07    64   239   721    47    45    40   134   151   237   112   168   158
       room64x16-filter5-t12      1.65e-05 4.2e-08 3.9e-07 1.9e-06  0.00  1.06 2.4e-07    64   239   721     0    44    40    96   182   278   118   140   130
       room333x10-quirk-t0        9.51e-05 4.5e-08 4.3e-07 1.9e-06  0.00  1.45 1.3e-07   210   783  2337   168   168   126   501   515   747   394   543   511
       room333x10-quirk-t12       9.51e-05 4.5e-08 4.3e-07 1.9e-06  0.00  1.45 6.4e-07   210   783  2337     0   147   126   417   641   852   436   469   427
       room333x10-offset0-t0      9.51e-05 4.5e-08 4.3e-07 1.9e-06  0.00  1.45 1.3e-07   210   783  2337   168   168   126   501   515   747   394   543   511
       room333x10-offset0-t12     9.51e-05 4.5e-08 4.3e-07 1.9e-06  0.00  1.45 6.4e-07   210   783  2337     0   147   126   417   641   852   436   469   427
       room333x10-nolabels-t0     9.51e-05 4.5e-08 4.3e-07 1.9e-06  0.00  1.45 6.4e-07   210   783  2337     0   147   126   417     0     0     0     0     0
       room333x10-nolabels-t12    9.51e-05 4.5e-08 4.3e-07 1.9e-06  0.00  1.45 6.4e-07   210   783  2337     0   147   126   417     0     0     0     0     0
       room333x10-filter0-t0      9.51e-05 4.5e-08 4.3e-07 2.0e-06  0.54  1.43 3.1e-07   210   783  2319     -     8     8   434  1148    67    58   122   120 k1b 0.27
       room333x10-filter0-t12     9.51e-05 4.5e-08 4.3e-07 2.0e-06  0.00  1.43 3.1e-07   210   783  2337     -     8     8   364  1208    67    58   122   120 k1b 0.27
       room333x10-filter1-t0      9.51e-05 4.5e-08 5.0e-07 2.0e-06  0.00  1.29 1.4e-07   210   783  2337     -   168   126   501  1040    63    55   128   127 k1b 0.29
       room333x10-filter1-t12     9.51e-05 4.5e-08 5.0e-07 2.0e-06  0.00  1.29 1.4e-07   210   783  2337     -   147   126   417  1208    63    55   128   127 k1b 0.29
       room333x10-filter2-t0      9.51e-05 4.5e-08 4.1e-07 2.0e-06  0.00  1.19 4.5e-07   210   783  2337   168   150   129   631   620   422   209  1168  1063 k1c 5.82e-06
       room333x10-filter2-t12     9.51e-05 4.5e-08 4.1e-07 2.1e-06  0.00  1.30 4.4e-07   210   783  2337     0    87    87   463   641   521   176  1150  1018 k1c 4.69e-06
       room333x10-filter3-t0      9.51e-05 4.5e-08 3.9e-07 2.2e-06  0.00  1.10 1.4e-07   210   783  2337   168   168   126   501   515   782   431   445   439 k1c 5.01e-06
       room333x10-filter3-t12     9.51e-05 4.5e-08 3.7e-07 1.8e-06  0.00  1.16 1.8e-07   210   783  2337     0   147   126   417   641   890   493   337   332 k1c 4.74e-06
       room333x10-filter4-t0      9.51e-05 4.5e-08 4.5e-07 1.8e-06  0.00  1.21 2.7e-07   210   783  2337     -     0     3   419  1208    85    57   105   103 k1c 6.92e-06
       room333x10-filter4-t12     9.51e-05 4.5e-08 4.3e-07 1.9e-06  0.00  1.34 1.4e-07   210   783  2337     -     0     3   335  1208    88    56   102   101 k1c 5.88e-06
       room333x10-filter5-t0      9.51e-05 4.5e-08 4.3e-07 1.9e-06  0.00  1.45 1.3e-07   210   783  2337   168   168   126   501   515   747   394   543   511
       room333x10-filter5-t12     9.51e-05 4.5e-08 4.3e-07 1.9e-06  0.00  1.45 6.4e-07   210   783  2337     0   147   126   417   641   852   436   469   427
       room70x9-quirk-t0          2.02e-05 4.2e-08 4.0e-07 1.8e-06  0.00  1.00 1.7e-07    45   145   440    30    31    26   112   115   130    68   118   111
       room70x9-quirk-t12         2.02e-05 4.2e-08 4.0e-07 1.8e-06  0.00  1.14 3.4e-07    45   145   440     0    30    25    90   136   153    74   104    95
       room70x9-offset0-t0        2.02e-05 4.2e-08 4.0e-07 1.8e-06  0.00  1.00 1.7e-07    45   145   440    30    31    26   112   115   130    68   118   111
       room70x9-offset0-t12       2.02e-05 4.2e-08 4.0e-07 1.8e-06  0.00  1.14 3.4e-07    45   145   440     0    30    25    90   136   153    74   104    95
       room70x9-nolabels-t0       2.02e-05 4.2e-08 4.0e-07 1.8e-06  0.00  1.14 3.4e-07    45   145   440     0    30    25    90     0     0     0     0     0
       room70x9-nolabels-t12      2.02e-05 4.2e-08 4.0e-07 1.8e-06  0.00  1.14 3.4e-07    45   145   440     0    30    25    90     0     0     0     0     0
       room70x9-filter0-t0        2.02e-05 4.2e-08 4.3e-07 1.7e-06  0.63  1.00 1.3e-07    45   145   436     -     3     3    93   225    10    14    53    52 k1b 0.19
       room70x9-filter0-t12       2.02e-05 4.2e-08 4.3e-07 1.7e-06  0.00  1.00 1.3e-07    45   145   440     -     3     3    77   239    10    14    53    52 k1b 0.19
       room70x9-filter1-t0        2.02e-05 4.2e-08 4.5e-07 1.6e-06  0.00  1.21 1.3e-07    45   145   440     -    31    26   112   209    15    18    44    43 k1b 0.27
       room70x9-filter1-t12       2.02e-05 4.2e-08 4.5e-07 2.0e-06  0.00  1.21 1.3e-07    45   145   440     -    30    25    90   239    15    18    44    43 k1b 0.27
       room70x9-filter2-t0        2.02e-05 4.2e-08 4.4e-07 1.6e-06  0.00  1.18 1.3e-07    45   145   440    30    29    33   137   130    74    27   232   217 k1c 5.02e-06
       room70x9-filter2-t12       2.02e-05 4.2e-08 4.1e-07 1.4e-06  0.00  0.95 1.2e-07    45   145   440     0    17    23   104   136    96    35   219   191 k1c 4.45e-06
       room70x9-filter3-t0        2.02e-05 4.2e-08 3.8e-07 1.8e-06  0.00  1.18 4.5e-07    45   145   440    30    31    26   112   115   136    62   115   111 k1c 3.72e-06
       room70x9-filter3-t12       2.02e-05 4.2e-08 3.5e-07 1.7e-06  0.00  1.16 6.6e-07    45   145   440     0    30    25    90   136   162    74    90    86 k1c 4.36e-06
       room70x9-filter4-t0        2.02e-05 4.2e-08 4.1e-07 1.7e-06  0.00  1.16 1.9e-07    45   145   440     -     0     3    90   239    18     9    50    49 k1c 4.58e-06
       room70x9-filter4-t12       2.02e-05 4.2e-08 4.6e-07 1.9e-06  0.00  1.01 1.1e-07    45   145   440     -     0     3    72   239    18     9    50    49 k1c 5.24e-06
       room70x9-filter5-t0        2.02e-05 4.2e-08 4.0e-07 1.8e-06  0.00  1.00 1.7e-07    45   145   440    30    31    26   112   115   130    68   118   111
       room70x9-filter5-t12       2.02e-05 4.2e-08 4.0e-07 1.8e-06  0.00  1.14 3.4e-07    45   145   440     0    30    25    90   136   153    74   104    95
       (worst over all: undecided 0.63 %, normal 1.45 of 8, K1b 0.29 of its bound, K1c 6.92e-06 m)

B. Small sizes (SMALL_IDS): the same construction at 23 x 5, 22 x 5, 16 x 4, 5 x 3 and 3 x 3 through K1 .. K3 and both
   filters -- below 23 columns the staging loop of k23_normals_labels wraps a column more than twice (it wrapped at most
   twice before this file existed, and read outside the row), below 13 the window of K1c revisits columns, as the
   shader's does.  The fp64 assertions of A hold on what fp64 decides (no census: 9 to 115 texels); on the GPU the
   frames are bit-equal to the oracle's.

C. Structural and branch rows (bit for bit against the oracle on the GPU; each with a property of its own, asserted on
   the oracle here and on the kernel there; whatever fp64 decides of a row is held as in A).
     corners                 points on texel corners and edges (fp64 coordinates within 1e-4 px of an integer): each lands
                             in the texel that the floor of the oracle's own fp32 coordinates names
     seam                    y = +0 and y = -0 at x < 0: column 0 by the specified atan2 (fp64's atan2 would say -pi, column W,
                             for -0: preprocess_ref states the specified one)
     gate-*-a / b            the two neighbouring fp32 inputs between which the ORACLE's outcome flips (bisection on the
                             oracle): range at min_depth and max_depth, z at fov_up and fov_down.  Precondition: fp64 puts
                             both within 2^-24 + two range steps of the clip / within the measured texel bound of the edge.
                             The clip is soft by design of `2 zn - 1`: a range 2.2e-6 m inside min_depth still rounds to -1
     clip-exact              ranges of exactly 2 and 75: z_ndc is exactly -1 and +1 and GL's closed cube keeps both
     tie-same-01 / -10       two ranges with the same 24-bit depth: the lower index wins, in both orders
     tie-quantum-02 / -20    two ranges one quantum apart: the nearer wins, in both orders
     one-texel-5000 (-avg)   5000 points in one texel: the nearest wins / the mean within n 2^-24 sum|terms|
     empty, empty-filters    no points: vertex 0, normal (0,0,0,1), semantic (0,0,0,1) (quirk B-2)
     n-255 / 256 / 257       around the 256-lane launch: texel k holds point k with its probability, nothing else is set
     bad-points              NaN, +-inf, the origin (range 0), 1e30, 1e-30: only the one good point lands
     tile-edges              130 x 17, a label edge on each side of every 64 x 8 tile and on the top and bottom rows: every
                             texel the erosion spares keeps its label
     seam-fill (-70)         labels in columns W-2, W-1 only: column 0 is filled across the seam at offset 1 (probability
                             / 2), column 1 at offset 2 (/ 3); at 70 columns the source sits in the overhanging tile's halo
     fill-threshold-side     a range step of 0.702 % around a gap: refused from the nearer side, filled from the farther
     eroded-source           two labels that erode each other beside a gap: the fill reads ERODED labels and finds nothing
     len-gate-below / above  |un x vn| one fp32 step either side of 1e-7 (differences exact by construction, bisection on the
                             oracle's normal.w): w = 0 / 1, the direction finite and of unit length on both sides
   The K1c window at rows 0 .. 5, H-6 .. H-1 and across the seam needs no row: every room scene has H <= 16 and wraps.

D. Mutations of oracle/o_preprocess.c on the CPU (scratch builds; the tests of this file that fail):
     `<=` -> `<` in the depth clip            clip-exact (the gate rows move with the oracle and cannot see it)
     the index dropped from the depth key     81 tests: every scene and small size with the depth test; 13 rows, among them
                                              tie-quantum-20, bad-points, clip-exact and the n rows (point 0 is read)
     o_wrap off by one (x == W stays)         106 tests: scenes and small sizes of every variant; seam-fill, seam-fill-70,
                                              tile-edges, eroded-source, fill-threshold-side, the n rows
     `ul != 0` dropped from the erosion       66 tests: every labelled scene without the blended scatter; seam-fill,
                                              seam-fill-70, fill-threshold-side, the n rows
     the fill's order, -x before +x           37 tests; +y / -y swapped: 45 tests (labelled scenes; the probability tells)
     `offset + 1` -> `offset`                 61 tests: labelled scenes without the blended scatter; seam-fill, seam-fill-70,
                                              tile-edges, fill-threshold-side
     the threshold on lq instead of lp        fill-threshold-side and 6 room scenes under K1c
     dynamic points counted in the average    the 12 room scenes filter0 / 1 / 4 at timestamp 0 (w must be 0 there)
     the K1c window not cut in y              39 tests: every scene and small size with K1c (edge rows fetched again)
   Equivalent: `&&` -> `||` in validity rule (1).  Rule (3) already invalidates when EITHER neighbour is not above 0.5,
   and every w that preprocessing can produce is 0, 0.25, 0.5 or 1 (K1b and K1c set w = 1 exactly wherever it exceeds
   0.5), so `w < 1` and `!(w > 0.5)` are the same predicate.
"""
from functools import lru_cache

import numpy as np
import pytest

import preprocess_ref as PR
from semantic_suma_amd.types import default_params

F32 = np.float32
U = PR.U
ROOM = dict(x=5.0, y=5.0, floor=-1.7, ceiling=3.0)
FLAT_RANGE = 6.0

# the parameter sets of FILTER_VARIANTS in tests/test_gpu_parity.py (that module is marked gpu as a whole, so the list is
# restated here; test_filter_variants_are_those_of_the_parity_file holds the two together)
FILTER_VARIANTS = [
    dict(avg_vertexmap=1),
    dict(avg_vertexmap=1, filter_sampling=1),
    dict(filter_vertexmap=1, use_filtered_vertexmap=1, bilateral_sigma_space=4.5, bilateral_sigma_range=2.5),
    dict(filter_vertexmap=1, use_filtered_vertexmap=1, bilateral_sigma_space=4.5, bilateral_sigma_range=2.5, filter_sampling=1),
    dict(avg_vertexmap=1, filter_vertexmap=1, use_filtered_vertexmap=1, bilateral_sigma_space=2.0, bilateral_sigma_range=0.5),
    dict(filter_vertexmap=1, use_filtered_vertexmap=0, bilateral_sigma_space=4.5),
]
VARIANTS = {"quirk": {}, "offset0": dict(label_offset=0, prob_offset=0), "nolabels": {}}
VARIANTS.update({f"filter{i}": ov for i, ov in enumerate(FILTER_VARIANTS)})
ROOM_SIZES = ((48, 12), (64, 16), (333, 10), (70, 9))
SMALL_SIZES = ((23, 5), (22, 5), (16, 4), (5, 3), (3, 3))
TIMESTAMPS = (0, 12)
ROW_EPS_SCENE = "room333x10-quirk-t12"


def scene_id(W, H, variant, t):
    return f"room{W}x{H}-{variant}-t{t}"


ROOM_IDS = [scene_id(W, H, v, t) for (W, H) in ROOM_SIZES for v in VARIANTS for t in TIMESTAMPS]
# the widths below tile + halo of K2 + K3 (and below the 13 columns of K1c's window): K1 .. K3 and both filters
SMALL_IDS = [scene_id(W, H, v, 12 if v.startswith("filter") else 0) for (W, H) in SMALL_SIZES
             for v in ("quirk", "offset0", "filter0", "filter1", "filter2", "filter3", "filter4")]

# 2 x the oracle's worst deviation from fp64 over all room scenes (the header table); see check_frame
K1C_MEASURED = 6.92e-6  # m, room64x16-filter2 (the header table)
K1C_RANGE_BOUND = 2 * K1C_MEASURED


def params(W, H, **ov):
    base = dict(data_width=W, data_height=H, model_width=W, model_height=H)
    base.update(ov)
    return default_params(**base)


def _lds(a, b, ii, jj):
    """fixed low-discrepancy pattern in [0, 1)"""
    return np.modf(a * ii + b * jj + 0.123)[0]


# ---------------------------------------------------------------------------------------------------------------------
# the room, texel by texel
# ---------------------------------------------------------------------------------------------------------------------
BLOCK_LABELS = (40.0, 50.0, 70.0, 72.0, 44.0, 48.0)  # none dynamic
DYNAMIC_PATCH, ISLAND = 30.0, 81.0


def texel_layout(W, H):
    """what every texel of a room scene is meant to hold, in periods of 16 columns and 8 rows (so that label edges fall
    on columns 63|64 and rows 7|8, the borders of the K2 + K3 tile):
      count    points in the texel, 1 .. 4; 0 in a motif over columns 0 .. 2 of a period (rows in threes: E V V / V V E /
               V E V) that gives every validity rule of K2 a texel it alone invalidates
      label    one label per 16 x 8 block; unlabelled gaps of 1 (column 3), 3 (6 .. 8) and 5 (10 .. 14) columns: the fill
               takes offset 1, offset 2, and finds nothing; a 2 x 3 patch of a dynamic class (columns 4, 5, rows 1 .. 3); a
               single-texel island (column 9, row 5)
      range    the room's planes in columns 0, 1 of a period, a constant 6 m (+- 0.05 %) elsewhere so that the fill's
               range test passes with a wide margin -- except, in odd periods, a step of 1.5 % between columns 3 and 4
               (the gap of 1 has one side within 0.7 % and one beyond) and, in the periods 2 mod 4, a spike of 2 % on
               columns 7 and 12 (every labelled neighbour is refused)"""
    ii, jj = np.meshgrid(np.arange(W), np.arange(H))
    cx, ry, per = ii % 16, jj % 8, ii // 16
    count = 1 + (7 * ii + 3 * jj + (ii * jj) % 3) % 4
    r3 = jj % 3
    empty = ((r3 == 0) & (cx == 0)) | ((r3 == 1) & (cx == 2)) | ((r3 == 2) & (cx == 1))
    count = np.where(empty, 0, count)
    label = np.asarray(BLOCK_LABELS)[(per + 2 * (jj // 8)) % len(BLOCK_LABELS)]
    label = np.where((cx == 3) | ((cx >= 6) & (cx <= 8)) | ((cx >= 10) & (cx <= 14)), 0.0, label)
    label = np.where(((cx == 4) | (cx == 5)) & (ry >= 1) & (ry <= 3), DYNAMIC_PATCH, label)
    label = np.where((cx == 9) & (ry == 5), ISLAND, label)
    scale = 1.0 + 0.0005 * _lds(0.7548776662, 0.5698402910, ii, jj)
    scale = np.where((per % 2 == 1) & (cx >= 4), scale * 1.015, scale)
    scale = np.where((per % 4 == 2) & ((cx == 7) | (cx == 12)), scale * 1.02, scale)
    flat = cx >= 2
    return dict(count=count, label=label, flat=flat, scale=scale)


def room_range(d):
    """distance from the origin to the room's planes along the unit directions d (.. x 3)"""
    with np.errstate(divide="ignore"):
        sx, sy = ROOM["x"] / np.abs(d[..., 0]), ROOM["y"] / np.abs(d[..., 1])
        sz = np.where(d[..., 2] < 0, ROOM["floor"] / d[..., 2], ROOM["ceiling"] / d[..., 2])
    return np.minimum(np.minimum(sx, sy), np.where(np.isfinite(sz) & (sz > 0), sz, np.inf))


def direction(p, u, v):
    """unit direction of the continuous texel coordinates (u, v): the inverse of K1's projection"""
    W, H = p.data_width, p.data_height
    fov_up, fov = abs(float(p.data_fov_up)), abs(float(p.data_fov_up)) + abs(float(p.data_fov_down))
    yaw = np.pi * (1.0 - 2.0 * np.asarray(u, dtype=np.float64) / W)
    elev = np.deg2rad(fov_up - (1.0 - np.asarray(v, dtype=np.float64) / H) * fov)
    return np.stack([np.cos(elev) * np.cos(yaw), np.cos(elev) * np.sin(yaw), np.sin(elev)], axis=-1)


def room_scan(p, with_labels=True, layout=None, seed=5):
    """points generated FROM texels: `count` points per texel, each at a fractional offset in [0.15, 0.85] of the texel
    in both directions, the ranges inside a texel 0.4 % (>= 16 mm) apart, the order shuffled by a fixed permutation.
    Labels and probabilities are laid out so that, read through the quirk offsets, point i receives its texel's label."""
    W, H = p.data_width, p.data_height
    lay = layout or texel_layout(W, H)
    xs, ys, ks = [], [], []
    for k in range(4):
        jj, ii = np.nonzero(lay["count"] > k)
        xs.append(ii), ys.append(jj), ks.append(np.full(ii.shape, k))
    ii, jj, kk = (np.concatenate(a) for a in (xs, ys, ks))
    fu = 0.15 + 0.7 * _lds(0.6180339887, 0.3247179572, ii + 0.37 * kk, jj)
    fv = 0.15 + 0.7 * _lds(0.2207440846, 0.8191725134, ii, jj + 0.61 * kk)
    d = direction(p, ii + fu, jj + fv)
    # which of the texel's points is the nearest varies with the texel
    rank = (kk + ii + 2 * jj) % np.maximum(lay["count"][jj, ii], 1)
    # on the planes the nearest point lies on its plane and the others 0.4 % per rank behind the texel's farthest hit
    on_plane = room_range(d)
    far = np.zeros((H, W))
    np.maximum.at(far, (jj, ii), on_plane)
    base = np.where(lay["flat"][jj, ii], FLAT_RANGE * lay["scale"][jj, ii], np.where(rank == 0, on_plane, far[jj, ii]))
    rng = base * (1.0 + 0.004 * rank)
    n = ii.size
    perm = np.random.default_rng(seed).permutation(n)
    pts = np.ones((n, 4), dtype=F32)
    pts[:, :3] = (rng[:, None] * d)[perm]
    if not with_labels:
        return pts, None, None
    lo, po = int(p.label_offset), int(p.prob_offset)
    lab_of, prob_of = lay["label"][jj, ii][perm], (0.5 + 0.45 * _lds(0.7071, 0.3141, ii, jj + 0.3 * kk))[perm]
    labels, probs = np.full(n, 99.0, dtype=F32), np.full(n, 0.125, dtype=F32)
    labels[lo:] = lab_of[:n - lo]
    probs[po:] = prob_of[:n - po]
    return pts, labels, probs


@lru_cache(maxsize=None)
def get_scene(sid):
    if sid in ROWS:
        return ROWS[sid]()
    size, variant, t = sid[4:].split("-")
    W, H = (int(s) for s in size.split("x"))
    p = params(W, H, **VARIANTS[variant])
    pts, labels, probs = room_scan(p, with_labels=variant != "nolabels")
    return dict(id=sid, params=p, pts=pts, labels=labels, probs=probs, timestamp=int(t[1:]), variant=variant)


# ---------------------------------------------------------------------------------------------------------------------
# the oracle
# ---------------------------------------------------------------------------------------------------------------------
def oracle():
    from oracle import pyoracle
    pyoracle.build()
    return pyoracle


def oracle_run(sc, ora=None):
    """(vertex, normal, semantic) of the oracle"""
    ora = ora or oracle().Oracle(sc["params"])
    f = ora.preprocess(sc["pts"], sc["labels"], sc["probs"], sc["timestamp"], ora.frame())
    return tuple(f.map(m).copy() for m in range(3))


@lru_cache(maxsize=None)
def oracle_results(sid):
    return oracle_run(get_scene(sid))


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def assert_frames_equal(got, want, what):
    for g, w, name in zip(got, want, ("vertex", "normal", "semantic")):
        ne = bits(g) != bits(w)
        assert not ne.any(), f"{what}.{name}: {int(ne.sum())} of {ne.size} words differ; first at {np.argwhere(ne)[:5].tolist()}"


# ---------------------------------------------------------------------------------------------------------------------
# fp64 and the bounds measured on the oracle
# ---------------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def fp64_k1(sid):
    sc = get_scene(sid)
    p = sc["params"]
    if p.avg_vertexmap:
        return PR.k1_sum_fp64(p, sc["pts"], sc["labels"], sc["probs"], sc["timestamp"])
    return PR.k1_fp64(p, sc["pts"], sc["labels"], sc["probs"], sc["timestamp"])


@lru_cache(maxsize=None)
def measured_eps(sid):
    """2 x the largest |oracle - fp64| of each compared term over the scene (the factor 2: the other side of the
    comparison carries an error of the same size); the texel coordinates get one fp32 ulp of the largest coordinate on
    top, for the floor.  The oracle's terms come from oracle/debug/o_preprocess_terms.c."""
    sc = get_scene(sid)
    p = sc["params"]
    ora = oracle().Oracle(p)
    pt = fp64_k1(sid)["points"]
    t = ora.debug_preprocess_point_terms(sc["pts"]).astype(np.float64)
    ok = pt["inside"]
    dev = lambda a, b: float(np.max(np.abs(a[ok] - b[ok]))) if ok.any() else 0.0
    d_tex = max(dev(t[:, 0], pt["u"]), dev(t[:, 1], pt["v"]))
    d_zn = dev(t[:, 2], pt["zn"])
    V = oracle_results(sid)[0]
    mt = ora.debug_preprocess_map_terms(V).astype(np.float64)
    k2 = PR.k2_fp64(V, np.zeros_like(V))
    k3lp = np.linalg.norm(V[..., :3].astype(np.float64), axis=-1)
    val = k2["valid"] & np.isfinite(k2["len"])
    d_len = float(np.max(np.abs(mt[..., 0][val] - k2["len"][val]))) if val.any() else 0.0
    # the flood-fill difference |lp - lq| - 0.007 lp of horizontally and vertically adjacent texels, as fp32 forms it
    lp32 = mt[..., 1].astype(F32)
    d_fill = 0.0
    for dx, dy in ((1, 0), (2, 0), (0, 1), (0, 2)):
        lq32, lq = PR._shift(lp32[..., None], dx, dy)[..., 0], PR._shift(k3lp[..., None], dx, dy)[..., 0]
        t32 = (np.abs(lp32 - lq32) - F32(0.007) * lp32).astype(np.float64)
        t64 = np.abs(k3lp - lq) - PR.FILL_THRESHOLD * k3lp
        d_fill = max(d_fill, float(np.max(np.abs(t32 - t64))))
    ulp = float(np.spacing(F32(max(p.data_width, p.data_height))))
    eps = dict(texel=2 * d_tex + ulp, zn=2 * d_zn, len=2 * d_len, fill=2 * d_fill)
    if sid in ROWS:  # a row of a few points measures little: no bound below the widest room scene's
        wide = measured_eps(ROW_EPS_SCENE)
        eps = {k: max(v, wide[k]) for k, v in eps.items()}
    return eps


def stage_fp64(sid, frame_vertex):
    """fp64's own run of the scene.  Without filters K2 / K3 read fp64's K1.  With a filter on they read the vertex map
    of the FRAME under test (held against fp64's filtered map first, check_frame): a filtered vertex carries a
    deviation of its own, and the normal of two such vertices a centimetre apart would carry it a thousandfold."""
    sc = get_scene(sid)
    p = sc["params"]
    k1 = fp64_k1(sid)
    filt = dict(V=None, bound=None)
    if p.avg_vertexmap:
        V = PR.k1b_fp64(k1["vsum"], p.filter_sampling)
        S = k1["ssum"]
        # n 2^-24 sum|terms|: n = the points in the (up to four) texels fetched, the four products and sums of the
        # fetch, the reciprocal and the product of the division
        nterm = PR.fetch_fp64(k1["landed"][..., None].astype(np.float64), p.filter_sampling)[..., 0] * \
            (1 if p.filter_sampling == PR.NEAREST else 4) + 6
        f = PR.fetch_fp64(k1["vsum"], p.filter_sampling)
        fa = PR.fetch_fp64(k1["asum"], p.filter_sampling)
        with np.errstate(divide="ignore", invalid="ignore"):
            bound = nterm[..., None] * U * np.where(f[..., 3:4] > 0.5, fa / f[..., 3:4], fa)
        filt = dict(V=V, bound=bound, stage="k1b")
    else:
        V, S = k1["V"], k1["S"]
    if p.filter_vertexmap and p.use_filtered_vertexmap:
        Vf, fr = PR.k1c_fp64(V, p.filter_sampling, p.bilateral_sigma_space, p.bilateral_sigma_range)
        filt = dict(V=Vf, range=fr, stage="k1c")
    Vk = V if filt["V"] is None else np.asarray(frame_vertex, dtype=np.float64)
    k2 = PR.k2_fp64(Vk, S)
    k3 = PR.k3_fp64(Vk, k2["eroded"])
    return dict(k1=k1, V=V, S=S, filt=filt, k2=k2, k3=k3)


def check_frame(sid, frame, who, caps=True):
    """the assertions of a room scene on the maps `frame` = (vertex, normal, semantic) of `who` (the oracle here, the
    kernel on the GPU).  Returns the measured figures."""
    sc = get_scene(sid)
    p = sc["params"]
    W, H = p.data_width, p.data_height
    Vg, Ng, Sg = (np.asarray(m, dtype=F32) for m in frame)
    eps = measured_eps(sid)
    st = stage_fp64(sid, Vg)
    k1, k2, k3 = st["k1"], st["k2"], st["k3"]
    avg = bool(p.avg_vertexmap)
    fig = dict(eps=eps)
    # --- K1
    pt = k1["points"]
    if avg:
        # no winner to decide: every point that lands counts.  A point within the bound of a texel edge or of the clip
        # taints the texels around it
        near = pt["finite"] & ((pt["m_texel"] <= eps["texel"]) | (pt["m_clip"] <= eps["zn"] + pt["zn_step"]))
        taint = np.zeros((H, W), dtype=bool)
        for i in np.flatnonzero(near):
            taint[np.clip(int(np.floor(pt["v"][i])), 0, H - 1), int(np.floor(pt["u"][i])) % W] = True
        dec1 = ~PR.spread(taint, 1)
    else:
        dec1 = PR.k1_decided(p, k1, eps["texel"], eps["zn"])
    if st["filt"]["V"] is None:
        # the oracle gives fp64's winner: the vertex is that point's coordinates, exactly
        ne = (bits(Vg) != bits(st["V"].astype(F32))).any(axis=-1)
        assert not (ne & dec1).any(), f"{who}: {int((ne & dec1).sum())} decided texels hold another point than fp64's winner; first at {np.argwhere(ne & dec1)[:5].tolist()}"
        decV = dec1
    elif st["filt"]["stage"] == "k1b":
        decV = ~PR.spread(~dec1, 1) if p.filter_sampling != PR.NEAREST else dec1
        want = st["filt"]["V"]
        assert np.array_equal(Vg[..., 3][decV], want[..., 3][decV].astype(F32)), f"{who}: K1b w differs from fp64's"
        err = np.abs(Vg[..., :3].astype(np.float64) - want[..., :3])
        b = st["filt"]["bound"][..., :3]
        bad = (err > b) & decV[..., None]
        fig["k1b_ratio"] = float(np.max(np.where(decV[..., None] & (b > 0), err / np.where(b > 0, b, 1.0), 0.0)))
        assert not bad.any(), f"{who}: K1b mean beyond n 2^-24 sum|terms| at {np.argwhere(bad)[:5].tolist()}"
    else:
        decV = ~PR.spread(~dec1, 7)
        want, fr = st["filt"]["V"], st["filt"]["range"]
        assert np.array_equal(Vg[..., 3][decV], want[..., 3][decV].astype(F32)), f"{who}: K1c w differs from fp64's"
        act = decV & np.isfinite(fr)
        got_r = np.linalg.norm(Vg[..., :3].astype(np.float64), axis=-1)
        dev = np.abs(got_r - fr)[act]
        fig["k1c_dev"] = float(dev.max()) if dev.size else 0.0
        assert fig["k1c_dev"] <= K1C_RANGE_BOUND, f"{who}: K1c range off by {fig['k1c_dev']:.3g} > {K1C_RANGE_BOUND:.3g}"
        # the direction is the unfiltered ray: 8 2^-24 relative on each component, on top of the range's bound
        derr = np.abs(Vg[..., :3].astype(np.float64) - want[..., :3])
        dbound = K1C_RANGE_BOUND + 8 * U * np.abs(want[..., :3])
        assert not ((derr > dbound) & act[..., None]).any(), f"{who}: K1c vertex beyond its bound"
    # --- K2 / K3 read texels up to 3 away (fill at 2, erosion one further)
    dec = ~PR.spread(~decV, 3) & (k2["m_len"] > eps["len"]) & ~(k3["m_fill"] <= eps["fill"])
    # a texel whose fill source's gate is undecided: the source's erosion needs no margin (labels are exact)
    fig["undecided"] = float(1.0 - dec.mean())
    if caps:
        assert fig["undecided"] <= 0.02, f"{who}: {100 * fig['undecided']:.2f} % of the texels undecided"
    # normals
    nb = PR.normal_bound(k2)
    assert np.array_equal(Ng[..., 3][dec], k2["normal"][..., 3][dec].astype(F32)), f"{who}: normal validity differs from fp64's at {np.argwhere((Ng[..., 3] != k2['normal'][..., 3]) & dec)[:5].tolist()}"
    val = dec & k2["valid"] & (k2["normal"][..., 3] > 0)
    nerr = np.abs(Ng[..., :3].astype(np.float64) - k2["normal"][..., :3])
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(val[..., None], np.where(nb > 0, nerr / (nb / 8.0), np.where(nerr > 0, np.inf, 0.0)), 0.0)
    fig["normal_ratio"] = float(ratio.max()) if val.any() else 0.0
    fig["normal_dev"] = float(nerr[val].max()) if val.any() else 0.0
    assert fig["normal_ratio"] <= 8.0, f"{who}: normal off by {fig['normal_ratio']:.2f} x 2^-24 sum|terms| (bound 8)"
    inval = dec & ~(k2["valid"])
    assert not Ng[..., :3][inval].any(), f"{who}: an invalid normal is not zero"
    # labels: exact, the probability up to the one division
    if not avg:
        want = k3["refined"]
        assert np.array_equal(Sg[..., :3][dec], want[..., :3][dec].astype(F32)), f"{who}: label / fill outcome differs from fp64's at {np.argwhere((Sg[..., 0] != want[..., 0].astype(F32)) & dec)[:5].tolist()}"
        perr = np.abs(Sg[..., 3].astype(np.float64) - want[..., 3])
        assert not ((perr > U * np.abs(want[..., 3])) & dec).any(), f"{who}: probability off by more than the one division"
    # outcomes among the decided
    count = k1["landed"] if avg else k1["count"]
    out = dict(empty=(count == 0), single=(count == 1), contested=(count > 1), rule1=k2["r1"], rule2=k2["r2"], rule3=k2["r3"],
               eroded=k2["was_eroded"], fill1=k3["fill"] == 1, fill2=k3["fill"] == 2, refused=k3["refused"],
               all_refused=k3["all_refused"])
    if not avg:
        out["dropped"] = k1["dropped"]
    fig["outcomes"] = {k: int((m & dec).sum()) for k, m in out.items()}
    return fig


def expected_outcomes(sc):
    """the outcomes a scene's parameter set allows: no labels, no label outcomes; the drop only on a first scan; under
    the blended scatter the labels are sums and are held to the oracle in bits only"""
    p = sc["params"]
    filtered = p.avg_vertexmap or (p.filter_vertexmap and p.use_filtered_vertexmap)
    names = ["empty", "single", "contested"]
    if not (filtered and p.filter_sampling != PR.NEAREST):  # the GL-initial fetch smears the holes the rules need
        names += ["rule1", "rule2", "rule3"]
    if sc["labels"] is not None and not sc["params"].avg_vertexmap:
        names += ["eroded", "fill1", "fill2", "refused", "all_refused"]
        if sc["timestamp"] < 10:
            names += ["dropped"]
    return names


# ---------------------------------------------------------------------------------------------------------------------
# structural and branch rows
# ---------------------------------------------------------------------------------------------------------------------
ROWS = {}


def row(name):
    def deco(fn):
        ROWS[name] = lambda: dict(id=name, variant="row", **fn())
        return fn
    return deco


def _scene(p, pts, labels=None, probs=None, timestamp=12, **more):
    pts = np.asarray(pts, dtype=F32).reshape(-1, 4)
    return dict(params=p, pts=pts, labels=None if labels is None else np.asarray(labels, dtype=F32),
                probs=None if probs is None else np.asarray(probs, dtype=F32), timestamp=timestamp, **more)


def point_at(p, u, v, rng=FLAT_RANGE):
    d = direction(p, u, v)
    out = np.ones(np.shape(u) + (4,), dtype=F32)
    out[..., :3] = np.asarray(rng)[..., None] * d
    return out


def landed(frame):
    """{(x, y): xyz} of the valid texels of a vertex map"""
    V = frame[0]
    return {(int(x), int(y)): tuple(V[y, x, :3]) for y, x in np.argwhere(V[..., 3] > 0)}


@row("corners")
def _corners():
    """points whose fp64 coordinates are integers in u, in v, and in both: each lands in the texel that the floor of
    the oracle's own fp32 coordinates names (the property), one per texel, so nothing competes"""
    p = params(48, 12)
    u = np.asarray([3.0, 7.5, 11.0, 20.0, 24.0, 33.0, 40.5, 47.0])
    v = np.asarray([2.5, 4.0, 6.0, 1.0, 6.0, 9.5, 11.0, 3.0])
    return _scene(p, point_at(p, u, v))


@row("seam")
def _seam():
    """y = +0 and y = -0 at x < 0: the specified atan2 gives +pi for both, column 0; rows 2 and 9"""
    p = params(48, 12)
    a, b = point_at(p, 0.0, 2.5)[None], point_at(p, 0.0, 9.5)[None]
    a[0, 1], b[0, 1] = 0.0, -0.0
    assert a[0, 0] < 0 and np.signbit(b[0, 1])
    return _scene(p, np.concatenate([a, b]))


def _ordered(x):
    """fp32 -> an integer that orders like the float"""
    i = int(np.asarray(x, dtype=F32).view(np.int32))
    return i if i >= 0 else -(i & 0x7fffffff)


def _unordered(k):
    return np.asarray(k if k >= 0 else (-k) | 0x80000000, dtype=np.uint32).view(F32)[()]


def _bisect(flips, lo, hi):
    """the two neighbouring fp32 values between lo and hi across which flips(x) changes"""
    li, hi_i = _ordered(lo), _ordered(hi)
    a, b = flips(_unordered(li)), flips(_unordered(hi_i))
    assert a != b, "the outcome is the same at both ends"
    while hi_i - li > 1:
        mid = (li + hi_i) // 2
        if flips(_unordered(mid)) == a:
            li = mid
        else:
            hi_i = mid
    return _unordered(li), _unordered(hi_i)


def _lands(p, pt4):
    ora = oracle().Oracle(p)
    f = ora.preprocess(np.asarray(pt4, dtype=F32).reshape(1, 4), None, None, 12, ora.frame())
    return bool((f.map(0)[..., 3] > 0).any())


GATES = ("min_depth", "max_depth", "fov_up", "fov_down")


@lru_cache(maxsize=None)
def gate_points(name):
    """the two fp32 inputs, neighbours, between which the ORACLE's outcome flips (bisection on the oracle): a range
    along a fixed direction for the depth clip, a z coordinate at fixed x, y for the field of view"""
    p = params(48, 12)
    d = direction(p, 10.37, 5.41).astype(F32)
    if name in ("min_depth", "max_depth"):
        g = float(p.min_depth if name == "min_depth" else p.max_depth)
        mk = lambda s: np.asarray([F32(s) * d[0], F32(s) * d[1], F32(s) * d[2], 1.0], dtype=F32)
        a, b = _bisect(lambda s: _lands(p, mk(s)), g * 0.9, g * 1.1)
    else:
        ang = np.deg2rad(abs(float(p.data_fov_up)) if name == "fov_up" else -abs(float(p.data_fov_down)))
        xy = FLAT_RANGE * np.asarray([np.cos(1.0), np.sin(1.0)])
        mk = lambda z: np.asarray([xy[0], xy[1], z, 1.0], dtype=F32)
        z0 = FLAT_RANGE * np.tan(ang)
        a, b = _bisect(lambda z: _lands(p, mk(z)), z0 - 0.5, z0 + 0.5)
    return p, mk(a), mk(b)


for _g in GATES:
    for _k, _side in enumerate(("a", "b")):
        ROWS[f"gate-{_g}-{_side}"] = (lambda g=_g, k=_k: dict(id=f"gate-{g}-{'ab'[k]}", variant="row",
                                                             **_scene(gate_points(g)[0], gate_points(g)[1 + k])))


@lru_cache(maxsize=None)
def tie_ranges():
    """three fp32 ranges along one direction: r0 and r1 quantise to the same 24-bit depth, r2 is the first that gives
    the next one (read from the oracle's own window depth)"""
    p = params(48, 12)
    ora = oracle().Oracle(p)
    d = direction(p, 20.4, 6.6).astype(F32)

    def d24(s):
        pt = np.asarray([[F32(s) * d[0], F32(s) * d[1], F32(s) * d[2], 1.0]], dtype=F32)
        t = ora.debug_preprocess_point_terms(pt)
        return int(ora.debug_depth24(t[:, 2])[0]), pt[0], (int(np.floor(t[0, 0])), int(np.floor(t[0, 1])))
    r = [F32(6.0)]
    base = d24(r[0])
    s = r[0]
    while True:
        s = np.nextafter(s, F32(np.inf))
        k = d24(s)
        if k[0] == base[0] and len(r) == 1 and (k[1] != base[1]).any():
            r.append(s)
        if k[0] == base[0] + 1:
            r.append(s)
            break
        assert k[0] <= base[0] + 1
    assert len(r) == 3, "the direction's fp32 ranges skip a quantum: pick another"
    pts = [d24(x)[1] for x in r]
    assert len({d24(x)[2] for x in r}) == 1, "the three points must share a texel"
    return p, pts, d24(r[0])[2]


for _name, _order in (("tie-same-01", (0, 1)), ("tie-same-10", (1, 0)), ("tie-quantum-02", (0, 2)), ("tie-quantum-20", (2, 0))):
    ROWS[_name] = (lambda n=_name, o=_order: dict(id=n, variant="row", order=o,
                                                   **_scene(tie_ranges()[0], np.stack([tie_ranges()[1][k] for k in o]))))


@row("one-texel-5000")
def _one_texel():
    """5000 points in one texel, the nearest in the middle of the index range; under the blended scatter the same cloud
    is one run of 5000 terms (row one-texel-5000-avg)"""
    p = params(48, 12)
    pts = np.tile(point_at(p, 30.5, 6.5)[None], (5000, 1))
    scale = 1.0 + 1e-4 * ((np.arange(5000) * 37) % 5000) / 5000.0
    pts[:, :3] = (pts[:, :3].astype(np.float64) * scale[:, None]).astype(F32)
    return _scene(p, pts)


@row("one-texel-5000-avg")
def _one_texel_avg():
    sc = _one_texel()
    sc["params"] = params(48, 12, avg_vertexmap=1, filter_sampling=1)
    return sc


@row("empty")
def _empty():
    return _scene(params(48, 12), np.zeros((0, 4), dtype=F32))


@row("empty-filters")
def _empty_f():
    return _scene(params(48, 12, **FILTER_VARIANTS[4]), np.zeros((0, 4), dtype=F32))


def _n_points(n):
    p = params(48, 12, label_offset=0, prob_offset=0)
    k = np.arange(n)
    pts = point_at(p, (k % 48) + 0.5, (k // 48) % 12 + 0.5, FLAT_RANGE + 0.01 * (k // 576))
    return _scene(p, pts, labels=np.full(n, 40.0), probs=0.5 + 0.001 * (k % 400))


for _n in (255, 256, 257):
    ROWS[f"n-{_n}"] = (lambda n=_n: dict(id=f"n-{n}", variant="row", **_n_points(n)))


@row("bad-points")
def _bad():
    """NaN and inf coordinates, the origin (range 0), and one good point: only the good one lands"""
    p = params(48, 12)
    g = point_at(p, 12.5, 3.5)
    bad = [[np.nan, 1, 1, 1], [1, np.nan, 1, 1], [1, 1, np.nan, 1], [np.inf, 1, 1, 1], [1, -np.inf, 1, 1], [1, 1, np.inf, 1],
           [np.inf, np.inf, np.inf, 1], [0, 0, 0, 1], [-0.0, -0.0, -0.0, 1], [0, 0, 5, 1], [1e30, 1e30, 1e30, 1],
           [1e-30, 0, 0, 1]]
    return _scene(p, np.concatenate([np.asarray(bad, dtype=F32), g[None]]))


def _labelled_grid(W, H, label_fn, variant=None, timestamp=12, range_fn=None):
    """one point at the centre of every texel, range 6 m, labels by label_fn(ii, jj)"""
    p = params(W, H, label_offset=0, prob_offset=0, **(variant or {}))
    ii, jj = np.meshgrid(np.arange(W), np.arange(H))
    rng = np.full((H, W), FLAT_RANGE) if range_fn is None else range_fn(ii, jj)
    pts = point_at(p, ii + 0.5, jj + 0.5, rng).reshape(-1, 4)
    lab = label_fn(ii, jj).astype(np.float64).ravel()
    return _scene(p, pts, labels=lab, probs=0.25 + 0.5 * _lds(0.31, 0.17, ii, jj).ravel(), timestamp=timestamp,
                  label_map=lab.reshape(H, W))


@row("tile-edges")
def _tile_edges():
    """130 x 17: a label edge across each side of every 64 x 8 tile (columns 63|64, 127|128, rows 7|8, 15|16) and on the
    image's top and bottom rows: exactly the two texels either side of an edge are eroded, everywhere"""
    return _labelled_grid(130, 17, lambda ii, jj: 40.0 + 2 * (ii // 64) + 10 * ((jj + 0) // 8) + 100 * ((jj == 0) | (jj == 16)))


@row("seam-fill")
def _seam_fill():
    """labels in columns W-2, W-1 only: column 0 is filled across the seam at offset 1 (from -x), column 1 at offset 2"""
    return _labelled_grid(48, 6, lambda ii, jj: np.where(ii >= 46, 50.0, 0.0))


@row("seam-fill-70")
def _seam_fill70():
    """the same where the tile overhangs the image (70 columns: the second tile's halo is columns 61 .. 69, 0 .. 62)"""
    return _labelled_grid(70, 6, lambda ii, jj: np.where(ii >= 68, 50.0, 0.0))


@row("clip-exact")
def _clip_exact():
    """ranges of exactly min_depth and max_depth (2 and 75 along an axis: the length is exact, z_ndc is exactly -1 and
    +1): GL clips against the CLOSED cube, both points land"""
    p = params(48, 12)
    assert float(p.min_depth) == 2.0 and float(p.max_depth) == 75.0
    return _scene(p, [[0.0, -2.0, 0.0, 1.0], [0.0, 75.0, 0.0, 1.0]])


@row("fill-threshold-side")
def _fill_threshold_side():
    """the range test is relative to the texel being filled (0.007 lp), not to its neighbour: around the unlabelled
    column 4 the ranges differ by 0.702 %.  Rows 0 .. 2: the gap is the NEARER side, |lp - lq| = 0.00702 lp: refused.
    Rows 3 .. 5: the gap is the farther side, |lp - lq| = 0.00697 lp: filled.  Either decision is 1.2e-4 m from its
    gate, some seventy times the measured bound"""
    far = lambda ii, jj: FLAT_RANGE * np.where((ii == 4) == (jj >= 3), 1.00702, 1.0)
    return _labelled_grid(48, 6, lambda ii, jj: np.where(ii == 4, 0.0, 50.0), range_fn=far)


@row("eroded-source")
def _eroded_source():
    """columns 5 | 6 carry two labels and erode each other; column 7 is unlabelled.  The fill reads ERODED labels, so
    column 7 finds nothing at offset 1 (column 6) nor at offset 2 (column 5) and stays 0, although both raw labels are
    set; column 3 likewise on the other side"""
    return _labelled_grid(48, 6, lambda ii, jj: np.where(ii == 5, 50.0, np.where(ii == 6, 70.0, 0.0)))


@lru_cache(maxsize=None)
def len_gate_points():
    """p, its right neighbour u = p + d and the texel above, v = p - d + (0, e, 0), with d = (0, -2^-6, -2^-4) and p.y =
    2^-7, so that every difference is exact in fp32: at e = 0 the two unit vectors are exact negatives and the cross
    product is exactly 0.  e moves |un x vn| by about 15 e; the two neighbouring fp32 values of v.y between which the
    ORACLE's normal.w flips are found by bisection.  Returns (params, points below, points above, the texel of p)."""
    p = params(48, 12)
    fov_up, fov = abs(float(p.data_fov_up)), abs(float(p.data_fov_up)) + abs(float(p.data_fov_down))
    elev = np.deg2rad(fov_up - (1.0 - 5.8 / 12) * fov)
    pz = np.round(4.0 * np.tan(elev) * 1024) / 1024
    P = np.asarray([4.0, 2.0 ** -7, pz])
    d = np.asarray([0.0, -2.0 ** -6, -2.0 ** -4])

    def mk(vy):
        pts = np.ones((4, 4), dtype=F32)
        pts[0, :3], pts[1, :3], pts[2, :3] = P, P + d, P - d
        pts[2, 1] = vy
        pts[3] = point_at(p, 23.5, 4.5)  # the texel below: rule (2) wants s or t valid
        assert np.array_equal(pts[:2, :3].astype(np.float64), np.stack([P, P + d]))
        return pts
    ora = oracle().Oracle(p)

    def valid(vy):
        f = ora.preprocess(mk(vy), None, None, 12, ora.frame())
        return float(f.map(1)[5, 23, 3]) == 1.0
    y0 = F32(3 * 2.0 ** -7)
    a, b = _bisect(valid, y0, y0 + F32(1e-6))
    return p, mk(a), mk(b), (23, 5)


for _k, _side in enumerate(("below", "above")):
    ROWS[f"len-gate-{_side}"] = (lambda k=_k: dict(id=f"len-gate-{('below', 'above')[k]}", variant="row",
                                                   **_scene(len_gate_points()[0], len_gate_points()[1 + k])))


def run_rows_property(sid, frame):
    """each row's own property, asserted on a result (the oracle's here, the kernel's on the GPU)"""
    sc = get_scene(sid)
    p = sc["params"]
    V, N, S = frame
    got = landed(frame)
    if sid == "corners":
        t = oracle().Oracle(p).debug_preprocess_point_terms(sc["pts"])
        want = {(int(np.floor(a)), int(np.floor(b))) for a, b, _ in t}
        assert set(got) == want and len(want) == len(sc["pts"])
        pt = PR.k1_points(p, sc["pts"])
        assert float(pt["m_texel"].max()) < 1e-4, "the points are meant to sit on texel edges"
    elif sid == "seam":
        assert set(got) == {(0, 2), (0, 9)}, got
    elif sid.startswith("gate-"):
        name, side = sid[5:].rsplit("-", 1)
        _, a, b = gate_points(name)
        la, lb = _lands(p, a), _lands(p, b)
        assert la != lb and bool(got) == (la if side == "a" else lb)
        pt = PR.k1_points(p, np.stack([a, b]))
        # precondition: fp64 puts both inputs within 8 ulps of the gate
        if name.endswith("depth"):
            g = float(p.min_depth if name == "min_depth" else p.max_depth)
            # 2^-24: `2 zn - 1` rounds to +-1 within half an ulp of 1; and two fp32 steps of the range
            assert np.all(pt["m_clip"] < U + 2 * float(np.spacing(F32(g))) / float(p.max_depth - p.min_depth))
        else:
            edge = p.data_height if name == "fov_up" else 0.0
            assert np.all(np.abs(pt["v"] - edge) < measured_eps("room48x12-quirk-t12")["texel"])
    elif sid.startswith("tie-"):
        _, pts, texel = tie_ranges()
        o = sc["order"]
        assert list(got) == [texel]
        winner = 0 if sid.startswith("tie-same") else o.index(0)  # same depth24: the lower index; else the nearer
        assert got[texel] == tuple(sc["pts"][winner, :3]), (sid, got, sc["pts"])
    elif sid == "one-texel-5000":
        k = int(np.argmin(np.linalg.norm(sc["pts"][:, :3].astype(np.float64), axis=1)))
        assert list(got) == [(30, 6)] and got[(30, 6)] == tuple(sc["pts"][k, :3])
    elif sid == "one-texel-5000-avg":
        assert list(got) == [(30, 6)]
        mean = sc["pts"][:, :3].astype(np.float64).mean(axis=0)
        assert np.all(np.abs(np.asarray(got[(30, 6)], dtype=np.float64) - mean) <= 5000 * U * np.abs(sc["pts"][:, :3].astype(np.float64)).mean(axis=0))
    elif sid in ("empty", "empty-filters"):
        assert not V.any() and not N[..., :3].any() and (N[..., 3] == 1).all() and (S[..., 3] == 1).all() and not S[..., :3].any()
    elif sid.startswith("n-"):
        n = int(sid[2:])
        flat = V.reshape(-1, 4)
        # one point per texel in raster order: texel k holds point k, with its own label and probability
        assert np.array_equal(flat[:n, :3], sc["pts"][:, :3]) and (flat[:n, 3] == 1).all() and not flat[n:].any()
        assert np.array_equal(S.reshape(-1, 4)[:n, 3], sc["probs"])
        assert len(got) == n
    elif sid == "bad-points":
        assert list(got) == [(12, 3)]
    elif sid == "tile-edges":
        L = sc["label_map"]
        ero = np.zeros(L.shape, dtype=bool)
        ero[:, :-1] |= L[:, :-1] != L[:, 1:]
        ero[:, 1:] |= L[:, :-1] != L[:, 1:]
        ero[:, 0] |= L[:, 0] != L[:, -1]
        ero[:, -1] |= L[:, 0] != L[:, -1]
        ero[:-1] |= L[:-1] != L[1:]
        ero[1:] |= L[:-1] != L[1:]
        # an eroded texel with an uneroded neighbour of a constant-range grid is filled again at offset 1 or 2: what is
        # asserted is the complement -- a texel the erosion spares keeps its own label and probability untouched
        keep = ~ero
        assert np.array_equal(S[..., 0][keep], (L / 255.0).astype(F32)[keep])
        assert ero.sum() > 400
    elif sid in ("seam-fill", "seam-fill-70"):
        W = p.data_width
        l50 = F32(50.0 / 255.0)
        assert (S[:, 0, 0] == l50).all() and (S[:, 1, 0] == l50).all() and (S[:, 2, 0] == 0).all()
        assert (S[:, W - 3, 0] == l50).all() and (S[:, W - 4, 0] == l50).all() and (S[:, W - 5, 0] == 0).all()
        probs = sc["probs"].reshape(p.data_height, W)
        assert np.array_equal(S[:, 0, 3], (probs[:, W - 1] / F32(2.0)).astype(F32))
        assert np.array_equal(S[:, 1, 3], (probs[:, W - 1] / F32(3.0)).astype(F32))
    elif sid == "clip-exact":
        assert len(got) == 2 and {v[1] for v in got.values()} == {-2.0, 75.0}, got
    elif sid == "fill-threshold-side":
        assert not S[:3, 4, :3].any() and (S[3:, 4, 0] == F32(50.0 / 255.0)).all(), S[:, 4]
    elif sid == "eroded-source":
        assert not S[..., :3].any(), "a fill took a raw label that the erosion had removed"
    elif sid.startswith("len-gate-"):
        assert set(got) == {(23, 5), (24, 5), (23, 6), (23, 4)}, got
        k2 = PR.k2_fp64(V, np.zeros_like(V))
        ln = float(k2["len"][5, 23])
        assert k2["valid"][5, 23] and abs(ln - PR.LEN_GATE) < 4e-8, ln  # one fp32 step of v.y moves len by 2.8e-8
        above = sid.endswith("above")
        assert float(N[5, 23, 3]) == (1.0 if above else 0.0) and (ln > PR.LEN_GATE) == above
        assert np.isfinite(N[5, 23, :3]).all() and abs(float(np.linalg.norm(N[5, 23, :3].astype(np.float64))) - 1) < 1e-6
    else:
        raise KeyError(sid)


ROW_IDS = list(ROWS)


# ---------------------------------------------------------------------------------------------------------------------
# the tests
# ---------------------------------------------------------------------------------------------------------------------
def _fmt(sid, fig):
    e, o = fig["eps"], fig["outcomes"]
    cols = ("empty", "single", "contested", "dropped", "rule1", "rule2", "rule3", "eroded", "fill1", "fill2", "refused", "all_refused")
    extra = f"k1b {fig['k1b_ratio']:.2f}" if "k1b_ratio" in fig else (f"k1c {fig['k1c_dev']:.2e}" if "k1c_dev" in fig else "")
    return (f"{sid:26s} {e['texel']:.2e} {e['zn']:.1e} {e['len']:.1e} {e['fill']:.1e} {100 * fig['undecided']:5.2f} "
            f"{fig['normal_ratio']:5.2f} {fig['normal_dev']:.1e} " + " ".join(f"{o.get(c, '-'):>5}" for c in cols) + " " + extra)


@pytest.mark.parametrize("sid", ROOM_IDS)
def test_room_scene_oracle_against_fp64(sid):
    sc = get_scene(sid)
    fig = check_frame(sid, oracle_results(sid), f"oracle {sid}")
    print(_fmt(sid, fig))
    for name in expected_outcomes(sc):
        assert fig["outcomes"][name] >= 10, f"{sid}: outcome {name} occurs {fig['outcomes'][name]} times among the decided"


@pytest.mark.parametrize("sid", SMALL_IDS)
def test_small_sizes_oracle_against_fp64(sid):
    """widths below tile + halo: the fp64 assertions hold (no outcome census: the images have 9 to 115 texels)"""
    fig = check_frame(sid, oracle_results(sid), f"oracle {sid}", caps=False)
    print(_fmt(sid, fig))


@pytest.mark.parametrize("sid", ROW_IDS)
def test_row_property(sid):
    run_rows_property(sid, oracle_results(sid))
    # and whatever fp64 decides of the row holds as in a room scene
    check_frame(sid, oracle_results(sid), f"oracle {sid}", caps=False)


def test_points_come_from_texels():
    """the construction: every point of a room scan lies 0.15 .. 0.85 into its texel, ranges within a texel are at
    least 1 mm apart, and the index order is not the raster order"""
    for (W, H) in ROOM_SIZES + SMALL_SIZES:
        p = params(W, H)
        pts, _, _ = room_scan(p)
        pt = PR.k1_points(p, pts)
        assert pt["inside"].all() and float(pt["m_texel"].min()) > 0.149
        pix = pt["ty"] * W + pt["tx"]
        assert (np.diff(pix) < 0).mean() > 0.3
        order = np.lexsort((pt["range"], pix))
        same = pix[order][1:] == pix[order][:-1]
        assert float(np.diff(pt["range"][order])[same].min()) > 1e-3
        assert set(np.bincount(pix, minlength=W * H)) == ({0, 1, 2, 3, 4} if W * H > 9 else {0, 2, 3, 4})


def test_w_channel_is_exact():
    """n * fl(1 / n) = 1 in binary32 for every count a scene can produce (the header of preprocess_ref.py)"""
    n = np.arange(1, 41, dtype=F32)
    assert np.all(n * (F32(1.0) / n) == F32(1.0))
    q = np.arange(1, 17, dtype=F32) / F32(4.0)  # the GL-initial fetch of counts up to 4
    assert np.all(q * (F32(1.0) / q) == F32(1.0))
    for sid in ROOM_IDS:
        if get_scene(sid)["params"].avg_vertexmap:
            assert int(fp64_k1(sid)["landed"].max()) <= 4


def test_filter_variants_are_those_of_the_parity_file():
    import ast
    import os
    src = open(os.path.join(os.path.dirname(__file__), "test_gpu_parity.py")).read()
    node = next(n for n in ast.parse(src).body if isinstance(n, ast.Assign) and n.targets[0].id == "FILTER_VARIANTS")
    assert eval(compile(ast.Expression(node.value), "variants", "eval")) == FILTER_VARIANTS
