* hand-written: 12 constraint rows over 6 variables, RANGES on a G row (R01), an L row (R02), an E row with positive R (R03)
* and an E row with negative R (R04).  Feasible at x = (2, 2, 3, 2, 3, 1); every variable in [0, 10].
NAME          RANGED
ROWS
 N  COST
 G  R01
 L  R02
 E  R03
 E  R04
 G  R05
 L  R06
 E  R07
 G  R08
 L  R09
 E  R10
 G  R11
 L  R12
COLUMNS
    X1        COST                 1.   R01                 1.
    X1        R02                  1.   R05                 1.
    X1        R07                  1.   R11                 1.
    X1        R12                  2.
    X2        COST                 2.   R01                 1.
    X2        R03                  1.   R07                -1.
    X2        R09                  1.   R11                 1.
    X3        COST                -1.   R02                 1.
    X3        R04                  1.   R09                 1.
    X3        R11                  1.
    X4        COST                 1.   R03                 1.
    X4        R06                  1.   R10                 1.
    X4        R11                  1.   R12                 1.
    X5        COST                -2.   R04                 1.
    X5        R06                  1.   R08                 1.
    X5        R10                 -1.   R11                 1.
    X6        COST                 1.   R05                 1.
    X6        R06                  1.   R07                 1.
    X6        R08                 -1.   R11                 1.
RHS
    B         R01                  2.   R02                 8.
    B         R03                  3.   R04                 6.
    B         R05                  1.   R06                12.
    B         R07                  1.   R08                -2.
    B         R09                  9.   R10                -1.
    B         R11                  5.   R12                10.
RANGES
    RNG       R01                  3.   R02                 4.
    RNG       R03                  2.   R04                -2.
BOUNDS
 UP BND       X1                  10.
 UP BND       X2                  10.
 UP BND       X3                  10.
 UP BND       X4                  10.
 UP BND       X5                  10.
 UP BND       X6                  10.
ENDATA
