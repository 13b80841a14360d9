from .vel_estimator import VelocityEstimator

__all__ = ["VelocityEstimator"]
