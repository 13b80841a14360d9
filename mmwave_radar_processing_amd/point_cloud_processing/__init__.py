from .vehicle_vel_estimator import VehicleVelEstimator
from .vel_estimator import VelocityEstimator

__all__ = ["VehicleVelEstimator", "VelocityEstimator"]
