from .inner_product_prover import NIProver, FastNIProver2
from .inner_product_verifier import Proof1, Proof2, Verifier1, Verifier2
from .batch import BatchInnerProductVerifier, batch_verify_inner_products, locate_by_bisection
from .batch_mixed import MixedBatchInnerProductVerifier, batch_verify_inner_products_mixed
from .batch_prover import BatchInnerProductProver
from .batch_prover_mixed import MixedBatchInnerProductProver

__all__ = ["NIProver", "FastNIProver2", "Proof1", "Proof2", "Verifier1", "Verifier2",
           "BatchInnerProductVerifier", "batch_verify_inner_products", "locate_by_bisection", "BatchInnerProductProver", "MixedBatchInnerProductProver",
           "MixedBatchInnerProductVerifier", "batch_verify_inner_products_mixed"]
