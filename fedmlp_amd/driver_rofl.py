#!/usr/bin/env python3
"""The RoFL row of the reference's main.py (:98-99, 167-168, 253-268, the branch it keeps commented out) on the HIP engine:
fedmlp_amd.driver's round loop with exp = "RoFL".  `python -m fedmlp_amd.driver --exp RoFL` stays refused (the driver's parser
lists the rows that are live in the reference); this module is the command for the row:

  python -m fedmlp_amd.driver_rofl --rounds_warmup 2 --n_local 64 --hw 64      # --forget_rate, --T_pl, --lambda_cen, --lambda_e

Every other flag is the driver's.  Per round: f_G (randn(2C, D) from a CPU generator seeded with --seed, the same on every rank)
goes to every client's train_RoFL; the clients' f_k reach every rank (all_gather_object); FedAvg; fedavg.rofl_centroids."""
from fedmlp_amd import driver


def args_parser(argv=None):
    p = driver.build_parser()
    p.set_defaults(exp="RoFL")
    args = p.parse_args(argv)
    if args.exp != "RoFL":
        p.error("fedmlp_amd.driver_rofl runs the RoFL row only; the other rows are fedmlp_amd.driver's")
    driver.check_drift_flags(p, args)             # --prox_mu / --scaffold: refused, train_RoFL installs no correction
    driver.check_server_flags(p, args)            # --server_opt: the driver's, RoFL aggregates with plain FedAvg
    return args


def main():
    return driver.main(args_parser(), module="fedmlp_amd.driver_rofl")


if __name__ == "__main__":
    main()
